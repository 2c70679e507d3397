// AmpSliceClient.hpp -- BufAmpSlice client over the MI355X C ABI (include/flucoma_hip.h).
//
// Mirrors the offline form of client::ampslice::AmpSliceClient, include/flucoma/clients/rt/AmpSliceClient.hpp:
//   parameter table  :39-48     fastRampUp / fastRampDown / slowRampUp / slowRampDown / onThreshold / offThreshold / floor /
//                               minSliceLength / highPassFreq, behind the slicing wrapper's source / startFrame / numFrames /
//                               startChan / numChans / indices (:112-114)
//   process          :77-96     one EnvelopeSegmentation::processSample per sample; hiPassFreq = min(highPassFreq /
//                               sampleRate, 0.5); latency :97 = 0
//   NRTAmpSliceClient / NRTThreadedAmpSliceClient  :116-120, behind NRTSliceAdaptor
//                               (clients/common/FluidNRTClientWrapper.hpp:665-725, SpikesToTimes.hpp)
// The whole job -- mono sum, hold, high-pass, level, followers, detector -- is one call, fluhip_bufampslice_f32.  There is
// no CPU path.
#pragma once

#include "NRTControlAdaptor.hpp"
#include "NRTThreadingAdaptor.hpp"
#include "ParamDescriptors.hpp"

namespace fluhip {
namespace ampslice {

enum AmpSliceParamIndex { // rt/AmpSliceClient.hpp:27-37
  kFastRampUpTime,
  kFastRampDownTime,
  kSlowRampUpTime,
  kSlowRampDownTime,
  kOnThreshold,
  kOffThreshold,
  kSilenceThreshold,
  kDebounce,
  kHiPassFreq
};

namespace detail {
inline double constrainDb(double v) { return std::min(144.0, std::max(-144.0, v)); } // Min(-144), Max(144)
} // namespace detail

struct NRTAmpSliceParams
{
  std::shared_ptr<const BufferAdaptor> source;        // "source"
  index                                startFrame{0}; // Min(0)
  index                                numFrames{-1};
  index                                startChan{0};  // Min(0)
  index                                numChans{-1};
  std::shared_ptr<BufferAdaptor>       indices;       // "indices"
  index                                fastRampUp{1};     // Min(1)
  index                                fastRampDown{1};   // Min(1)
  index                                slowRampUp{100};   // Min(1)
  index                                slowRampDown{100}; // Min(1)
  double                               onThreshold{144};   // Min(-144), Max(144)
  double                               offThreshold{-144}; // Min(-144), Max(144)
  double                               floor{-144};        // Min(-144), Max(144)
  index                                minSliceLength{2};  // Min(0)
  double                               highPassFreq{85};   // Min(0)

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
    fastRampUp = std::max<index>(1, fastRampUp);
    fastRampDown = std::max<index>(1, fastRampDown);
    slowRampUp = std::max<index>(1, slowRampUp);
    slowRampDown = std::max<index>(1, slowRampDown);
    onThreshold = detail::constrainDb(onThreshold);
    offThreshold = detail::constrainDb(offThreshold);
    floor = detail::constrainDb(floor);
    minSliceLength = std::max<index>(0, minSliceLength);
    highPassFreq = std::max(0.0, highPassFreq);
  }
};
} // namespace ampslice

class NRTAmpSliceClient
{
public:
  using ParamSetViewType = ampslice::NRTAmpSliceParams;
  static constexpr ParamDescriptorList getParameterDescriptors() { return paramdesc::list(paramdesc::kBufAmpSlice); }

  NRTAmpSliceClient(ParamSetViewType& p, FluidContext&) : mParams(&p) {}
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

    // a detection needs the value before it below the threshold: every other sample at most
    const int64_t        capacity = nFrames / 2 + 2;
    std::vector<int64_t> idx((size_t) capacity);
    int64_t              count = 0;
    const int rc = fluhip_bufampslice_f32(mDevice.get(), audio.data(), 1, nChans, nFrames, P.startFrame, P.fastRampUp,
                                          P.fastRampDown, P.slowRampUp, P.slowRampDown, P.onThreshold, P.offThreshold, P.floor,
                                          P.minSliceLength, P.highPassFreq, sampleRate, idx.data(), capacity, &count);
    if (rc != FLUHIP_OK) return mDevice.result(rc);
    if (count > capacity) return {S::kError, "more slices than samples allow"};
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

using NRTThreadedAmpSliceClient = NRTThreadingAdaptor<NRTAmpSliceClient>; // rt/AmpSliceClient.hpp:120

} // namespace fluhip
