// PitchClient.hpp -- BufPitch client over the MI355X C ABI (include/flucoma_hip.h).
//
// Mirrors the offline form of client::pitch::PitchClient, include/flucoma/clients/rt/PitchClient.hpp:
//   parameter table  :39-48     select / algorithm / minFreq / maxFreq / unit / fftSettings, behind the wrapper's
//                               source / startFrame / numFrames / startChan / numChans / features / padding (:180-182)
//   process          :93-150    STFT magnitude -> CepstrumF0 / HPS (nHarmonics 4) / YINFFT ::processFrame, the pitch in Hz or
//                               MIDI, the selected values as the output channels in order; latency :151 = the window
//   NRTPitchClient / NRTThreadedPitchClient  :184-188
// The whole job -- every channel, every frame -- is one call, fluhip_bufpitch_f32.  An empty selection is the library's
// announced error (the reference would write no channel at all).
#pragma once

#include "NRTControlAdaptor.hpp"
#include "NRTThreadingAdaptor.hpp"
#include "ParamDescriptors.hpp"

namespace fluhip {
namespace pitch {

enum PitchParamIndex { kSelect, kAlgorithm, kMinFreq, kMaxFreq, kUnit, kFFT }; // rt/PitchClient.hpp:30-37

struct NRTPitchParams : NRTControlParams
{
  index     select{3};       // ChoicesParam: bit 0 pitch, bit 1 confidence; all on by default
  index     algorithm{2};    // Cepstrum, Harmonic Product Spectrum, YinFFT
  double    minFreq{20};     // Min(0), Max(10000), UpperLimit<maxFreq>
  double    maxFreq{10000};  // Min(1), Max(20000), LowerLimit<minFreq>
  index     unit{0};         // Hz, MIDI
  FFTParams fftSettings{1024, -1, -1};

  index numSelected() const { return (select & 1) + ((select >> 1) & 1); }

  void constrain()
  {
    constrainWrapper();
    impl::constrainFFT(fftSettings);
    select &= 3;
    algorithm = std::min<index>(2, std::max<index>(0, algorithm));
    unit = std::min<index>(1, std::max<index>(0, unit));
    maxFreq = std::min(20000.0, std::max(1.0, maxFreq));
    minFreq = std::min(std::min(10000.0, std::max(0.0, minFreq)), maxFreq); // capped at maxFreq
    maxFreq = std::max(maxFreq, minFreq);                                   // floored at minFreq
  }
};
} // namespace pitch

class NRTPitchClient
{
public:
  using ParamSetViewType = pitch::NRTPitchParams;
  // the parameter table a host enumerates (rt/PitchClient.hpp:180-188; ParamDescriptors.hpp)
  static constexpr ParamDescriptorList getParameterDescriptors() { return paramdesc::list(paramdesc::kBufPitch); }

  NRTPitchClient(ParamSetViewType& p, FluidContext&) : mParams(&p) {}
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
                                    return fluhip_bufpitch_f32(ctx, audio, count, n, f.winSize(), f.fftSize(), f.hopSize(), padding,
                                                               (int) P.algorithm, P.minFreq, P.maxFreq, (int) P.unit,
                                                               (int) P.select, sampleRate, out, frames);
                                  });
  }

private:
  ParamSetViewType* mParams;
  DeviceContext     mDevice;
};

using NRTThreadedPitchClient = NRTThreadingAdaptor<NRTPitchClient>; // rt/PitchClient.hpp:188

} // namespace fluhip
