// NMFCrossClient.hpp -- BufNMFCross client over the MI355X C ABI (include/flucoma_hip.h).
//
// Mirrors client::nmfcross::NMFCrossClient, include/flucoma/clients/nrt/NMFCrossClient.hpp:26-191:
//   parameter table   :38-48    -> NMFCrossParams (plain struct, same names / defaults / constraints; constrain() applies
//                                  Min(1), Odd() (an even value becomes the next odd one) and FrameSizeUpperLimit<kFFT>
//                                  in the reference's order)
//   process           :84-184   -> same checks, messages and order; reads channel 0 of source and target, resizes the
//                                  output to tgtFrames x 1 at the SOURCE's sample rate; STFT + NMFCross + synthesis +
//                                  GriffinLim + ISTFT are one call, fluhip_bufnmfcross_f32; progress goes to the task
//                                  as processUpdate(count, iterations + 3) like the reference's callback (:146-180)
// The reference's sparsity / polyphony factor is 1 - ((i + 1) / iterations) in integer arithmetic: those two constraints act
// on the last iteration only (include/flucoma_hip.h, fluhip_nmfcross_process_f64).  There is no CPU path: if the library
// cannot create a context on the requested device the job returns kError.
#pragma once

#include "BufferAdaptor.hpp"
#include "ParamDescriptors.hpp"
#include "DeviceContext.hpp"
#include "NRTThreadingAdaptor.hpp"

#include <algorithm>
#include <memory>
#include <vector>

namespace fluhip {
namespace nmfcross {

// nrt/NMFCrossClient.hpp:26-36
enum NMFCrossParamIndex { kSource, kTarget, kOutput, kTimeSparsity, kPolyphony, kContinuity, kIterations, kRandomSeed, kFFT };

// nrt/NMFCrossClient.hpp:38-48
struct NMFCrossParams
{
  std::shared_ptr<const BufferAdaptor> source;           // "source"
  std::shared_ptr<const BufferAdaptor> target;           // "target"
  std::shared_ptr<BufferAdaptor>       output;           // "output"
  index                                timeSparsity{7};  // Min(1), Odd()
  index                                polyphony{11};    // Min(1), Odd(), FrameSizeUpperLimit<kFFT>()
  index                                continuity{7};    // Min(1), Odd()
  index                                iterations{50};   // Min(1)
  index                                seed{-1};
  FFTParams                            fftSettings{1024, -1, -1};

  template <class In, class Out>
  void forEachBuffer(In&& in, Out&& out)
  {
    forEachBuffer(in, out, out);
  }
  template <class In, class Out, class OutOnly>
  void forEachBuffer(In&& in, Out&&, OutOnly&& outOnly)
  {
    in(source);
    in(target);
    outOnly(output);
  }

  static index odd(index x) { return x % 2 ? x : x + 1; } // cc/ParameterConstraints.hpp Odd
  void constrain()
  {
    fftSettings.win = std::max<index>(4, fftSettings.win); // cc/ParameterTypes.hpp:371-393
    if (fftSettings.fft >= 0)
    {
      index p = 1;
      while (p < std::max(fftSettings.fft, fftSettings.win)) p <<= 1;
      fftSettings.fft = p;
    }
    timeSparsity = odd(std::max<index>(1, timeSparsity));
    polyphony = std::min<index>(odd(std::max<index>(1, polyphony)), fftSettings.frameSize());
    continuity = odd(std::max<index>(1, continuity));
    iterations = std::max<index>(1, iterations);
  }
};

class NMFCrossClient
{
public:
  using ParamSetViewType = NMFCrossParams;
  static constexpr ParamDescriptorList getParameterDescriptors() { return paramdesc::list(paramdesc::kBufNMFCross); }

  NMFCrossClient(NMFCrossParams& p, FluidContext&) : mParams(&p) {}
  void setParams(NMFCrossParams& p) { mParams = &p; }

  template <typename T>
  Result process(FluidContext& c)
  {
    using S = Result::Status;
    const NMFCrossParams& P = *mParams;
    BufferAdaptor::ReadAccess source(P.source.get());
    BufferAdaptor::ReadAccess target(P.target.get());
    BufferAdaptor::Access     output(P.output.get());
    const double              sampleRate = source.sampleRate();
    if (!source.exists()) return {S::kError, "Source Buffer Supplied But Invalid"}; // :94-99
    if (!target.exists()) return {S::kError, "Target Buffer Supplied But Invalid"};
    if (!output.exists()) return {S::kError, "Output Buffer Supplied But Invalid"};

    const index srcFrames = source.numFrames(), tgtFrames = target.numFrames();
    const index hop = P.fftSettings.hopSize();
    const index tgtWindows = (tgtFrames + hop) / hop; // :104-109
    if (srcFrames <= 0) return {S::kError, "Empty source buffer"};   // :111-118
    if (tgtFrames <= 0) return {S::kError, "Empty target buffer"};
    if (P.timeSparsity > tgtWindows) return {S::kError, "Time Sparsity is larger than target frames"};
    if (P.continuity > tgtWindows) return {S::kError, "Continuity is larger than target frames"};

    Result resizeResult = output.resize(tgtFrames, 1, sampleRate); // :133-134
    if (!resizeResult.ok()) return resizeResult;

    Result dev = mDevice.ensure(c.device());
    if (!dev.ok()) return dev;

    auto src = source.samps(0, srcFrames, 0);
    auto tgt = target.samps(0, tgtFrames, 0);
    std::vector<float> out((size_t) tgtFrames);
    struct Progress
    {
      FluidContext* c;
      double        total;
      static int cb(int64_t count, void* u)
      {
        auto* p = static_cast<Progress*>(u);
        return p->c->task() ? (p->c->task()->processUpdate(static_cast<double>(count), p->total) ? 1 : 0) : 1;
      }
    } prog{&c, static_cast<double>(P.iterations + 3)};
    const int rc = fluhip_bufnmfcross_f32(mDevice.get(), src.data(), srcFrames, src.stride, tgt.data(), tgtFrames, tgt.stride,
                                          P.fftSettings.winSize(), P.fftSettings.fftSize(), hop, P.timeSparsity, P.polyphony,
                                          P.continuity, P.iterations, P.seed, out.data(), &Progress::cb, &prog);
    if (rc != FLUHIP_OK) return mDevice.result(rc);
    output.samps(0) <<= VectorView<const float>(out.data(), tgtFrames); // :182
    return {};
  }

private:
  NMFCrossParams* mParams;
  DeviceContext   mDevice;
};
} // namespace nmfcross

using NRTNMFCrossClient = NRTThreadingAdaptor<nmfcross::NMFCrossClient>; // nrt/NMFCrossClient.hpp:188-190

} // namespace fluhip
