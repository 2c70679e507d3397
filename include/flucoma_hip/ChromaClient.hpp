// ChromaClient.hpp -- BufChroma client over the MI355X C ABI (include/flucoma_hip.h).
//
// Mirrors the offline form of client::chroma::ChromaClient, include/flucoma/clients/rt/ChromaClient.hpp:
//   parameter table  :36-42     numChroma / ref / normalize / minFreq / maxFreq / fftSettings, behind the wrapper's
//                               source / startFrame / numFrames / startChan / numChans / features / padding (:138-140)
//   process          :75-109    STFT magnitude -> ChromaFilterBank::processFrame, numChroma output channels; latency :111 =
//                               the window
//   NRTChromaClient / NRTThreadedChromaClient  :142-146
// The whole job -- every channel, every frame -- is one call, fluhip_bufchroma_f32.  The library takes numChroma up to 128
// and announces an error above (upstream the bound is a runtime maximum of the real-time object).
#pragma once

#include "NRTControlAdaptor.hpp"
#include "NRTThreadingAdaptor.hpp"
#include "ParamDescriptors.hpp"

namespace fluhip {
namespace chroma {

enum ChromaParamIndex { kNChroma, kRef, kNorm, kMinFreq, kMaxFreq, kFFT }; // rt/ChromaClient.hpp:27-34

struct NRTChromaParams : NRTControlParams
{
  index     numChroma{12}; // Min(2)
  double    ref{440};      // Min(0), Max(22000)
  index     normalize{0};  // None, Sum, Max
  double    minFreq{0};    // Min(0)
  double    maxFreq{-1};   // Min(-1); -1: half the sample rate
  FFTParams fftSettings{1024, -1, -1};

  void constrain()
  {
    constrainWrapper();
    impl::constrainFFT(fftSettings);
    numChroma = std::max<index>(2, numChroma);
    ref = std::min(22000.0, std::max(0.0, ref));
    normalize = std::min<index>(2, std::max<index>(0, normalize));
    minFreq = std::max(0.0, minFreq);
    maxFreq = std::max(-1.0, maxFreq);
  }
};
} // namespace chroma

class NRTChromaClient
{
public:
  using ParamSetViewType = chroma::NRTChromaParams;
  // the parameter table a host enumerates (rt/ChromaClient.hpp:138-146; ParamDescriptors.hpp)
  static constexpr ParamDescriptorList getParameterDescriptors() { return paramdesc::list(paramdesc::kBufChroma); }

  NRTChromaClient(ParamSetViewType& p, FluidContext&) : mParams(&p) {}
  void setParams(ParamSetViewType& p) { mParams = &p; }

  template <typename T>
  Result process(FluidContext& c)
  {
    const ParamSetViewType& P = *mParams;
    const FFTParams         f = P.fftSettings;
    const double            sampleRate = P.source ? BufferAdaptor::ReadAccess(P.source.get()).sampleRate() : 0.0;
    // (a channel count the library would refuse still reaches it: the announced error is the library's)
    const index nFeatures = std::min<index>(128, std::max<index>(1, P.numChroma));
    return impl::streamingControl(P, f, nFeatures, mDevice, c,
                                  [&](fluhip_ctx* ctx, const float* audio, int64_t count, int64_t n, int padding, float* out,
                                      int64_t* frames) {
                                    return fluhip_bufchroma_f32(ctx, audio, count, n, f.winSize(), f.fftSize(), f.hopSize(), padding,
                                                                P.numChroma, P.ref, (int) P.normalize, P.minFreq, P.maxFreq,
                                                                sampleRate, out, frames);
                                  });
  }

private:
  ParamSetViewType* mParams;
  DeviceContext     mDevice;
};

using NRTThreadedChromaClient = NRTThreadingAdaptor<NRTChromaClient>; // rt/ChromaClient.hpp:146

} // namespace fluhip
