// LoudnessClient.hpp -- BufLoudness client over the MI355X C ABI (include/flucoma_hip.h).
//
// Mirrors the offline form of client::loudness::LoudnessClient, include/flucoma/clients/rt/LoudnessClient.hpp:
//   parameter table  :36-45     select / kWeighting / truePeak / windowSize / hopSize / maxWindowSize, behind the wrapper's
//                               source / startFrame / numFrames / startChan / numChans / features / padding (:144-146)
//   process          :77-118    one Loudness::processFrame per hop on the window that ends there; the filter and the
//                               interpolator are never reset between frames; latency :120 = the window
//   NRTLoudnessClient / NRTThreadedLoudnessClient  :148-152
// maxWindowSize is fixed at construction upstream (it sizes the buffers): here it only caps windowSize.  The whole job -- every
// channel, every frame, the latency frames included -- is one call, fluhip_bufloudness_f32; channels go in as its `count` and
// share no state.  An empty selection is the library's announced error (the reference would write no channel at all).
#pragma once

#include "NRTControlAdaptor.hpp"
#include "NRTThreadingAdaptor.hpp"
#include "ParamDescriptors.hpp"

namespace fluhip {
namespace loudness {

enum LoudnessParamIndex { kSelect, kKWeighting, kTruePeak, kWindowSize, kHopSize, kMaxWindowSize }; // rt/LoudnessClient.hpp:27-34

struct NRTLoudnessParams : NRTControlParams
{
  index select{3};            // ChoicesParam: bit 0 loudness, bit 1 peak; both on
  index kWeighting{1};        // Off, On
  index truePeak{1};          // Off, On
  index windowSize{1024};     // Min(1), UpperLimit<maxWindowSize>
  index hopSize{512};         // Min(1)
  index maxWindowSize{16384}; // Fixed; Min(4), PowerOfTwo, Max(32768)

  index numSelected() const { return (select & 1) + (select >> 1 & 1); }

  void constrain()
  {
    constrainWrapper();
    select &= 3;
    kWeighting = std::min<index>(1, std::max<index>(0, kWeighting));
    truePeak = std::min<index>(1, std::max<index>(0, truePeak));
    // PowerOfTwo rounds up (cc/ParameterConstraints.hpp), then Min / Max clamp
    index p = 1;
    while (p < maxWindowSize && p < 32768) p <<= 1;
    maxWindowSize = std::min<index>(32768, std::max<index>(4, p));
    windowSize = std::min(maxWindowSize, std::max<index>(1, windowSize));
    hopSize = std::max<index>(1, hopSize);
  }
};
} // namespace loudness

class NRTLoudnessClient
{
public:
  using ParamSetViewType = loudness::NRTLoudnessParams;
  // the parameter table a host enumerates (rt/LoudnessClient.hpp:144-152; ParamDescriptors.hpp)
  static constexpr ParamDescriptorList getParameterDescriptors() { return paramdesc::list(paramdesc::kBufLoudness); }

  NRTLoudnessClient(ParamSetViewType& p, FluidContext&) : mParams(&p) {}
  void setParams(ParamSetViewType& p) { mParams = &p; }

  template <typename T>
  Result process(FluidContext& c)
  {
    using S = Result::Status;
    const ParamSetViewType& P = *mParams;
    // what the parameter set refuses upstream; announced here, in front of the wrapper's own arithmetic with the hop
    const index maxWin = P.maxWindowSize;
    if (maxWin < 4 || maxWin > 32768 || (maxWin & (maxWin - 1))) return {S::kError, "maxWindowSize must be a power of two from 4 to 32768"};
    if (P.windowSize < 1 || P.windowSize > maxWin) return {S::kError, "windowSize must be in [1, maxWindowSize]"};
    if (P.hopSize < 1) return {S::kError, "hopSize must be at least 1"};
    const FFTParams f(P.windowSize, P.hopSize, -1); // (the wrapper reads the window and the hop from it)
    const double    sampleRate = P.source ? BufferAdaptor::ReadAccess(P.source.get()).sampleRate() : 0.0;
    return impl::streamingControl(P, f, P.numSelected(), mDevice, c,
                                  [&](fluhip_ctx* ctx, const float* audio, int64_t count, int64_t n, int padding, float* out,
                                      int64_t* frames) {
                                    return fluhip_bufloudness_f32(ctx, audio, count, n, P.windowSize, P.hopSize, padding,
                                                                  (int) P.select, (int) P.kWeighting, (int) P.truePeak, sampleRate,
                                                                  out, frames);
                                  });
  }

private:
  ParamSetViewType* mParams;
  DeviceContext     mDevice;
};

using NRTThreadedLoudnessClient = NRTThreadingAdaptor<NRTLoudnessClient>; // rt/LoudnessClient.hpp:152

} // namespace fluhip
