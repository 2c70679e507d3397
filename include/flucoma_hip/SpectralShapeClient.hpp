// SpectralShapeClient.hpp -- BufSpectralShape client over the MI355X C ABI (include/flucoma_hip.h).
//
// Mirrors the offline form of client::spectralshape::SpectralShapeClient, include/flucoma/clients/rt/SpectralShapeClient.hpp:
//   parameter table  :39-47     select / minFreq / maxFreq / rolloffPercent / unit / power / fftSettings, behind the wrapper's
//                               source / startFrame / numFrames / startChan / numChans / features / padding (:150-153)
//   process          :88-127    STFT magnitude -> SpectralShape::processFrame, the selected descriptors as the output
//                               channels in table order; latency :129 = the window
//   NRTSpectralShapeClient / NRTThreadedSpectralShapeClient  :155-161
// The whole job -- every channel, every frame -- is one call, fluhip_bufspectralshape_f32.  An empty selection is the
// library's announced error (the reference would write no channel at all).
#pragma once

#include "NRTControlAdaptor.hpp"
#include "NRTThreadingAdaptor.hpp"
#include "ParamDescriptors.hpp"

namespace fluhip {
namespace spectralshape {

enum SpectralShapeParamIndex { kSelect, kMinFreq, kMaxFreq, kRollOffPercent, kFreqUnits, kAmpMeasure, kFFT }; // rt/SpectralShapeClient.hpp:29-37

struct NRTSpectralShapeParams : NRTControlParams
{
  index     select{127};        // ChoicesParam: bits 0 .. 6 centroid, spread, skew, kurtosis, rolloff, flatness, crest; all on
  double    minFreq{0};         // Min(0)
  double    maxFreq{-1};        // Min(-1); -1: half the sample rate
  double    rolloffPercent{95}; // Min(0), Max(100)
  index     unit{0};            // Hz, Midi Cents
  index     power{0};           // No, Yes
  FFTParams fftSettings{1024, -1, -1};

  index numSelected() const
  {
    index n = 0;
    for (int i = 0; i < 7; i++) n += (select >> i) & 1;
    return n;
  }

  void constrain()
  {
    constrainWrapper();
    impl::constrainFFT(fftSettings);
    select &= 127;
    minFreq = std::max(0.0, minFreq);
    maxFreq = std::max(-1.0, maxFreq);
    rolloffPercent = std::min(100.0, std::max(0.0, rolloffPercent));
    unit = std::min<index>(1, std::max<index>(0, unit));
    power = std::min<index>(1, std::max<index>(0, power));
  }
};
} // namespace spectralshape

class NRTSpectralShapeClient
{
public:
  using ParamSetViewType = spectralshape::NRTSpectralShapeParams;
  // the parameter table a host enumerates (rt/SpectralShapeClient.hpp:150-161; ParamDescriptors.hpp)
  static constexpr ParamDescriptorList getParameterDescriptors() { return paramdesc::list(paramdesc::kBufSpectralShape); }

  NRTSpectralShapeClient(ParamSetViewType& p, FluidContext&) : mParams(&p) {}
  void setParams(ParamSetViewType& p) { mParams = &p; }

  template <typename T>
  Result process(FluidContext& c)
  {
    const ParamSetViewType& P = *mParams;
    const FFTParams         f = P.fftSettings;
    const double            sampleRate = P.source ? BufferAdaptor::ReadAccess(P.source.get()).sampleRate() : 0.0;
    return impl::streamingControl(P, f, P.numSelected(), mDevice, c,
                                  [&](fluhip_ctx* ctx, const float* audio, int64_t count, int64_t n, int padding, float* out,
                                      int64_t* frames) {
                                    return fluhip_bufspectralshape_f32(ctx, audio, count, n, f.winSize(), f.fftSize(), f.hopSize(),
                                                                       padding, (int) P.select, P.minFreq, P.maxFreq,
                                                                       P.rolloffPercent, (int) P.unit, (int) P.power, sampleRate,
                                                                       out, frames);
                                  });
  }

private:
  ParamSetViewType* mParams;
  DeviceContext     mDevice;
};

using NRTThreadedSpectralShapeClient = NRTThreadingAdaptor<NRTSpectralShapeClient>; // rt/SpectralShapeClient.hpp:160-161

} // namespace fluhip
