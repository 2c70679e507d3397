// OnsetSliceClient.hpp -- BufOnsetSlice and BufOnsetFeature clients over the MI355X C ABI (include/flucoma_hip.h).
//
// Mirrors the offline forms of
//   client::onsetslice::OnsetSliceClient      include/flucoma/clients/rt/OnsetSliceClient.hpp:38-48 (parameters), :79-126
//                                             (process), :128 (latency: one hop), behind NRTSliceAdaptor
//                                             (clients/common/FluidNRTClientWrapper.hpp:665-725, SpikesToTimes.hpp)
//   client::onsetfeature::OnsetFeatureClient  include/flucoma/clients/rt/OnsetFeatureClient.hpp:29-37, :77-114, behind
//                                             NRTControlAdaptor (FluidNRTClientWrapper.hpp:551-660)
// The whole job -- mono sum, transforms, the metric, the running median, threshold and debounce -- is one call:
// fluhip_bufonsetslice_f32 / fluhip_bufonsetfeature_f32.  All ten metrics are built.  There is no CPU path.
#pragma once

#include "NRTControlAdaptor.hpp"
#include "NRTThreadingAdaptor.hpp"
#include "ParamDescriptors.hpp"

namespace fluhip {
namespace onsetslice {

enum OnsetParamIndex { kFunction, kThreshold, kDebounce, kFilterSize, kFrameDelta, kFFT }; // rt/OnsetSliceClient.hpp:29-36

namespace detail {
inline index constrainFilterSize(index f) // Min(1), Odd(), Max(101): an even value becomes the next odd one
{
  f = std::max<index>(1, f);
  if (f % 2 == 0) f++;
  return std::min<index>(101, f);
}
} // namespace detail

struct NRTOnsetSliceParams
{
  std::shared_ptr<const BufferAdaptor> source;        // "source"
  index                                startFrame{0}; // Min(0)
  index                                numFrames{-1};
  index                                startChan{0};  // Min(0)
  index                                numChans{-1};
  std::shared_ptr<BufferAdaptor>       indices;       // "indices"
  index                                metric{0};     // Energy .. Rectified Complex Domain
  double                               threshold{0.5}; // Min(0)
  index                                minSliceLength{2}; // Min(0)
  index                                filterSize{5}; // Min(1), Odd(), Max(101)
  index                                frameDelta{0}; // Min(0), Max(8192)
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
    outOnly(indices);
  }
  void constrain()
  {
    startFrame = std::max<index>(0, startFrame);
    startChan = std::max<index>(0, startChan);
    impl::constrainFFT(fftSettings);
    metric = std::min<index>(9, std::max<index>(0, metric));
    threshold = std::max(0.0, threshold);
    minSliceLength = std::max<index>(0, minSliceLength);
    filterSize = detail::constrainFilterSize(filterSize);
    frameDelta = std::min<index>(8192, std::max<index>(0, frameDelta));
  }
};
} // namespace onsetslice

namespace onsetfeature {

enum OnsetParamIndex { kFunction, kFilterSize, kFrameDelta, kFFT }; // rt/OnsetFeatureClient.hpp:27

struct NRTOnsetFeatureParams : NRTControlParams
{
  index     metric{0};
  index     filterSize{5}; // Min(1), Odd(), Max(101)
  index     frameDelta{0}; // Min(0), Max(8192)
  FFTParams fftSettings{1024, -1, -1};

  void constrain()
  {
    constrainWrapper();
    impl::constrainFFT(fftSettings);
    metric = std::min<index>(9, std::max<index>(0, metric));
    filterSize = onsetslice::detail::constrainFilterSize(filterSize);
    frameDelta = std::min<index>(8192, std::max<index>(0, frameDelta));
  }
};
} // namespace onsetfeature

class NRTOnsetSliceClient
{
public:
  using ParamSetViewType = onsetslice::NRTOnsetSliceParams;
  static constexpr ParamDescriptorList getParameterDescriptors() { return paramdesc::list(paramdesc::kBufOnsetSlice); }

  NRTOnsetSliceClient(ParamSetViewType& p, FluidContext&) : mParams(&p) {}
  void setParams(ParamSetViewType& p) { mParams = &p; }

  template <typename T>
  Result process(FluidContext& c)
  {
    using S = Result::Status;
    const ParamSetViewType& P = *mParams;
    // NRTClientWrapper::process, cc/FluidNRTClientWrapper.hpp:298-353
    index  nFrames = P.numFrames, nChans = P.numChans;
    Result rangeCheck = bufferRangeCheck(P.source.get(), P.startFrame, nFrames, P.startChan, nChans);
    if (!rangeCheck.ok()) return rangeCheck;
    if (!P.indices || !BufferAdaptor::Access(P.indices.get()).exists()) return {S::kError, "No valid output has been set"};

    Result dev = mDevice.ensure(c.device());
    if (!dev.ok()) return dev;

    BufferAdaptor::ReadAccess source(P.source.get());
    const double              sampleRate = source.sampleRate();
    std::vector<float>        audio((size_t) (nChans * nFrames));
    for (index i = 0; i < nChans; ++i)
      VectorView<float>(audio.data() + i * nFrames, nFrames) <<= source.samps(P.startFrame, nFrames, P.startChan + i);

    const FFTParams      f = P.fftSettings;
    const int64_t        capacity = nFrames / f.hopSize() + 2; // a detection per frame at most
    std::vector<int64_t> idx((size_t) capacity);
    int64_t              count = 0;
    const int rc = fluhip_bufonsetslice_f32(mDevice.get(), audio.data(), 1, nChans, nFrames, P.startFrame, (int) P.metric,
                                            P.threshold, P.minSliceLength, P.filterSize, P.frameDelta, f.winSize(), f.fftSize(),
                                            f.hopSize(), idx.data(), capacity, &count);
    if (rc != FLUHIP_OK) return mDevice.result(rc);
    if (count > capacity) return {S::kError, "more slices than frames"};
    if (FluidTask* task = c.task()) task->processUpdate(1.0, 1.0);

    // spikesToTimes: numSpikes x 1 at the source's sample rate (the single value -1 when nothing was detected)
    BufferAdaptor::Access out(P.indices.get());
    Result                resizeResult = out.resize(count, 1, sampleRate);
    if (!resizeResult.ok()) return resizeResult;
    std::vector<float> vals((size_t) count);
    for (int64_t i = 0; i < count; i++) vals[(size_t) i] = static_cast<float>(idx[(size_t) i]);
    out.samps(0) <<= VectorView<const float>(vals.data(), count);
    return {};
  }

private:
  ParamSetViewType* mParams;
  DeviceContext     mDevice;
};

class NRTOnsetFeatureClient
{
public:
  using ParamSetViewType = onsetfeature::NRTOnsetFeatureParams;
  static constexpr ParamDescriptorList getParameterDescriptors() { return paramdesc::list(paramdesc::kBufOnsetFeature); }

  NRTOnsetFeatureClient(ParamSetViewType& p, FluidContext&) : mParams(&p) {}
  void setParams(ParamSetViewType& p) { mParams = &p; }

  template <typename T>
  Result process(FluidContext& c)
  {
    using S = Result::Status;
    const ParamSetViewType& P = *mParams;
    index  nFrames = P.numFrames, nChans = P.numChans;
    Result rangeCheck = bufferRangeCheck(P.source.get(), P.startFrame, nFrames, P.startChan, nChans);
    if (!rangeCheck.ok()) return rangeCheck;
    if (!P.features || !BufferAdaptor::Access(P.features.get()).exists()) return {S::kError, "No valid output has been set"};

    Result dev = mDevice.ensure(c.device());
    if (!dev.ok()) return dev;

    BufferAdaptor::ReadAccess source(P.source.get());
    const double              sampleRate = source.sampleRate();
    std::vector<float>        audio((size_t) (nChans * nFrames));
    for (index i = 0; i < nChans; ++i)
      VectorView<float>(audio.data() + i * nFrames, nFrames) <<= source.samps(P.startFrame, nFrames, P.startChan + i);

    const FFTParams f = P.fftSettings;
    auto call = [&](float* out, int64_t* frames) {
      return fluhip_bufonsetfeature_f32(mDevice.get(), audio.data(), nChans, nFrames, (int) P.metric, P.filterSize, P.frameDelta,
                                        f.winSize(), f.fftSize(), f.hopSize(), (int) P.padding, out, frames);
    };
    int64_t keepHops = 0;
    int     rc = call(nullptr, &keepHops); // StreamingControl's frame bookkeeping (:564-579, 642-644), from the library
    if (rc != FLUHIP_OK) return mDevice.result(rc);
    std::vector<float> out((size_t) (nChans * keepHops));
    if ((rc = call(out.data(), &keepHops)) != FLUHIP_OK) return mDevice.result(rc);
    if (FluidTask* task = c.task()) task->processUpdate(1.0, 1.0);

    BufferAdaptor::Access thisOutput(P.features.get()); // :636-656, one feature per channel
    Result                resizeResult = thisOutput.resize(keepHops, nChans, sampleRate / f.hopSize());
    if (!resizeResult.ok()) return resizeResult;
    for (index j = 0; j < nChans; ++j) thisOutput.samps(j) <<= VectorView<const float>(out.data() + j * keepHops, keepHops);
    return {};
  }

private:
  ParamSetViewType* mParams;
  DeviceContext     mDevice;
};

using NRTThreadingOnsetSliceClient = NRTThreadingAdaptor<NRTOnsetSliceClient>;   // rt/OnsetSliceClient.hpp:160
using NRTThreadedOnsetFeatureClient = NRTThreadingAdaptor<NRTOnsetFeatureClient>; // rt/OnsetFeatureClient.hpp:145-146

} // namespace fluhip
