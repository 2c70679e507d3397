// NoveltySliceClient.hpp -- BufNoveltySlice and BufNoveltyFeature clients over the MI355X C ABI (include/flucoma_hip.h).
//
// Mirrors the offline forms of
//   client::noveltyslice::NoveltySliceClient      include/flucoma/clients/rt/NoveltySliceClient.hpp:44-53 (parameters),
//                                                 :128-192 (process), :194-201 (latency), behind NRTSliceAdaptor
//                                                 (clients/common/FluidNRTClientWrapper.hpp:665-725, SpikesToTimes.hpp)
//   client::noveltyfeature::NoveltyFeatureClient  include/flucoma/clients/rt/NoveltyFeatureClient.hpp:36-43, :120-191, behind
//                                                 NRTControlAdaptor (FluidNRTClientWrapper.hpp:551-660)
// The whole job -- mono sum, features, curve, smoothing, peaks -- is one call: fluhip_bufnoveltyslice_f32 /
// fluhip_bufnoveltyfeature_f32.  Algorithms Spectrum (0) and MFCC (1) are built; Chroma, Pitch and Loudness (2 - 4) return
// kError with a message that names the algorithm.  There is no CPU path.
#pragma once

#include "NRTControlAdaptor.hpp"
#include "NRTThreadingAdaptor.hpp"
#include "ParamDescriptors.hpp"

namespace fluhip {
namespace noveltyslice {

enum NoveltyParamIndex { kFeature, kKernelSize, kThreshold, kFilterSize, kDebounce, kFFT }; // rt/NoveltySliceClient.hpp:35-42

struct NRTNoveltySliceParams
{
  std::shared_ptr<const BufferAdaptor> source;        // "source"
  index                                startFrame{0}; // Min(0)
  index                                numFrames{-1};
  index                                startChan{0};  // Min(0)
  index                                numChans{-1};
  std::shared_ptr<BufferAdaptor>       indices;       // "indices"
  index                                algorithm{0};  // Spectrum, MFCC, Chroma, Pitch, Loudness
  index                                kernelSize{3}; // Min(3), Odd()
  double                               threshold{0.5}; // Min(0)
  index                                filterSize{1}; // Min(1)
  index                                minSliceLength{2}; // Min(0)
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
    algorithm = std::min<index>(4, std::max<index>(0, algorithm));
    kernelSize = std::max<index>(3, kernelSize);
    if (kernelSize % 2 == 0) kernelSize++; // Odd(): an even value becomes the next odd one
    threshold = std::max(0.0, threshold);
    filterSize = std::max<index>(1, filterSize);
    minSliceLength = std::max<index>(0, minSliceLength);
  }
};
} // namespace noveltyslice

namespace noveltyfeature {

enum NoveltyParamIndex { kFeature, kKernelSize, kFilterSize, kFFT }; // rt/NoveltyFeatureClient.hpp:34

struct NRTNoveltyFeatureParams : NRTControlParams
{
  index     algorithm{0};
  index     kernelSize{3}; // Min(3), Odd()
  index     filterSize{1}; // Min(1)
  FFTParams fftSettings{1024, -1, -1};

  void constrain()
  {
    constrainWrapper();
    impl::constrainFFT(fftSettings);
    algorithm = std::min<index>(4, std::max<index>(0, algorithm));
    kernelSize = std::max<index>(3, kernelSize);
    if (kernelSize % 2 == 0) kernelSize++;
    filterSize = std::max<index>(1, filterSize);
  }
};
} // namespace noveltyfeature

namespace impl {
inline index noveltyLatency(index hop, index kernelSize, index filterSize) // rt/NoveltySliceClient.hpp:194-201
{
  if (filterSize % 2) filterSize++;
  return hop * (1 + ((kernelSize + 1) >> 1) + (filterSize >> 1));
}
} // namespace impl

class NRTNoveltySliceClient
{
public:
  using ParamSetViewType = noveltyslice::NRTNoveltySliceParams;
  static constexpr ParamDescriptorList getParameterDescriptors() { return paramdesc::list(paramdesc::kBufNoveltySlice); }

  NRTNoveltySliceClient(ParamSetViewType& p, FluidContext&) : mParams(&p) {}
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
    const int rc = fluhip_bufnoveltyslice_f32(mDevice.get(), audio.data(), 1, nChans, nFrames, P.startFrame, (int) P.algorithm,
                                              P.kernelSize, P.threshold, P.filterSize, P.minSliceLength, f.winSize(), f.fftSize(),
                                              f.hopSize(), sampleRate, idx.data(), capacity, &count);
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

class NRTNoveltyFeatureClient
{
public:
  using ParamSetViewType = noveltyfeature::NRTNoveltyFeatureParams;
  static constexpr ParamDescriptorList getParameterDescriptors() { return paramdesc::list(paramdesc::kBufNoveltyFeature); }

  NRTNoveltyFeatureClient(ParamSetViewType& p, FluidContext&) : mParams(&p) {}
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
      return fluhip_bufnoveltyfeature_f32(mDevice.get(), audio.data(), nChans, nFrames, (int) P.algorithm, P.kernelSize,
                                          P.filterSize, f.winSize(), f.fftSize(), f.hopSize(), sampleRate, (int) P.padding, out,
                                          frames);
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

using NRTThreadingNoveltySliceClient = NRTThreadingAdaptor<NRTNoveltySliceClient>;   // rt/NoveltySliceClient.hpp:239-240
using NRTThreadedNoveltyFeatureClient = NRTThreadingAdaptor<NRTNoveltyFeatureClient>; // rt/NoveltyFeatureClient.hpp:235-236

} // namespace fluhip
