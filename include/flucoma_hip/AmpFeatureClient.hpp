// AmpFeatureClient.hpp -- BufAmpFeature client over the MI355X C ABI (include/flucoma_hip.h).
//
// Mirrors the offline form of client::ampfeature::AmpFeatureClient, include/flucoma/clients/rt/AmpFeatureClient.hpp:
//   parameter table  :36-42     fastRampUp / fastRampDown / slowRampUp / slowRampDown / floor / highPassFreq, behind the audio
//                               wrapper's source / startFrame / numFrames / startChan / numChans / features (:108-111); no
//                               padding parameter
//   process          :71-92     one Envelope::processSample per sample, the value cast to the host's float; latency :93 = 0
//   NRTAmpFeatureClient / NRTThreadedAmpFeatureClient  :113-116, behind NRTStreamAdaptor
//                               (clients/common/FluidNRTClientWrapper.hpp:466-548): every channel on its own through a reset
//                               client, the output numFrames x numChans at the source's sample rate
// The whole job -- every channel, every sample -- is one call, fluhip_bufampfeature_f32; the channels go in as independent
// signals and share no state.  There is no CPU path.
#pragma once

#include "AmpSliceClient.hpp"

namespace fluhip {
namespace ampfeature {

enum AmpFeatureParamIndex { // rt/AmpFeatureClient.hpp:27-34
  kFastRampUpTime,
  kFastRampDownTime,
  kSlowRampUpTime,
  kSlowRampDownTime,
  kSilenceThreshold,
  kHiPassFreq
};

struct NRTAmpFeatureParams
{
  std::shared_ptr<const BufferAdaptor> source;        // "source"
  index                                startFrame{0}; // Min(0)
  index                                numFrames{-1};
  index                                startChan{0};  // Min(0)
  index                                numChans{-1};
  std::shared_ptr<BufferAdaptor>       features;      // "features"
  index                                fastRampUp{1};     // Min(1)
  index                                fastRampDown{1};   // Min(1)
  index                                slowRampUp{100};   // Min(1)
  index                                slowRampDown{100}; // Min(1)
  double                               floor{-144};       // Min(-144), Max(144)
  double                               highPassFreq{85};  // Min(0)

  template <class In, class Out>
  void forEachBuffer(In&& in, Out&& out)
  {
    forEachBuffer(in, out, out);
  }
  template <class In, class Out, class OutOnly>
  void forEachBuffer(In&& in, Out&&, OutOnly&& outOnly)
  {
    in(source);
    outOnly(features);
  }
  void constrain()
  {
    startFrame = std::max<index>(0, startFrame);
    startChan = std::max<index>(0, startChan);
    fastRampUp = std::max<index>(1, fastRampUp);
    fastRampDown = std::max<index>(1, fastRampDown);
    slowRampUp = std::max<index>(1, slowRampUp);
    slowRampDown = std::max<index>(1, slowRampDown);
    floor = ampslice::detail::constrainDb(floor);
    highPassFreq = std::max(0.0, highPassFreq);
  }
};
} // namespace ampfeature

class NRTAmpFeatureClient
{
public:
  using ParamSetViewType = ampfeature::NRTAmpFeatureParams;
  static constexpr ParamDescriptorList getParameterDescriptors() { return paramdesc::list(paramdesc::kBufAmpFeature); }

  NRTAmpFeatureClient(ParamSetViewType& p, FluidContext&) : mParams(&p) {}
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

    std::vector<float> out((size_t) (nChans * nFrames));
    const int rc = fluhip_bufampfeature_f32(mDevice.get(), audio.data(), 1, nChans, nFrames, P.fastRampUp, P.fastRampDown,
                                            P.slowRampUp, P.slowRampDown, P.floor, P.highPassFreq, sampleRate, out.data());
    if (rc != FLUHIP_OK) return mDevice.result(rc);
    if (FluidTask* task = c.task()) task->processUpdate(1.0, 1.0);

    BufferAdaptor::Access thisOutput(P.features.get()); // Streaming::process :535-544
    Result                resizeResult = thisOutput.resize(nFrames, nChans, sampleRate);
    if (!resizeResult.ok()) return resizeResult;
    for (index j = 0; j < nChans; ++j) thisOutput.samps(j) <<= VectorView<const float>(out.data() + j * nFrames, nFrames);
    return {};
  }

private:
  ParamSetViewType* mParams;
  DeviceContext     mDevice;
};

using NRTThreadedAmpFeatureClient = NRTThreadingAdaptor<NRTAmpFeatureClient>; // rt/AmpFeatureClient.hpp:116

} // namespace fluhip
