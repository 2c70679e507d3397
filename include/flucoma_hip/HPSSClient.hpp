// HPSSClient.hpp -- BufHPSS over the MI355X C ABI (include/flucoma_hip.h).
//
// Mirrors the offline form of client::hpss::HPSSClient, include/flucoma/clients/rt/HPSSClient.hpp:37-48 (parameters),
// :80-84 (latency), :93-116 (process), behind NRTStreamAdaptor (:126-136; impl::Streaming, clients/common/
// FluidNRTClientWrapper.hpp:466-547): one audio input, three audio outputs -- harmonic, percussive, residual -- each its own
// buffer parameter, resized to numFrames x numChans at the source's sample rate; an output buffer that is absent is
// skipped, and with none at all the job is an error (:322-328).
// The whole job -- transforms, the two median filters, the masks, the three inverse transforms of every channel -- is one
// call, fluhip_bufhpss_f32.  There is no CPU path.
#pragma once

#include "NRTControlAdaptor.hpp"
#include "NRTThreadingAdaptor.hpp"
#include "ParamDescriptors.hpp"

#include <array>

namespace fluhip {
namespace hpss {

enum HPSSParamIndex { kHSize, kPSize, kMode, kHThresh, kPThresh, kFFT }; // rt/HPSSClient.hpp:28-35

// FloatPairsArrayT::type, cc/ParameterTypes.hpp:208-258: two (frequency, amplitude) pairs, (0, 1) and (1, 1) by default
struct FloatPairsArray
{
  std::array<std::pair<double, double>, 2> value{{{0.0, 1.0}, {1.0, 1.0}}};
  // FrequencyAmpPairConstraint at construction (cc/ParameterConstraints.hpp:235-268): frequencies clipped to [0, 1], a
  // pair in the wrong order swapped
  void constrain()
  {
    value[0].first = std::max(std::min(value[0].first, 1.0), 0.0);
    value[1].first = std::max(std::min(value[1].first, 1.0), 0.0);
    if (value[0].first > value[1].first) std::swap(value[0], value[1]);
  }
};

namespace detail {
inline index constrainFilterSize(index f) // Odd{}, Min(3): an even value becomes the next odd one
{
  f = std::max<index>(3, f);
  if (f % 2 == 0) f++;
  return f;
}
} // namespace detail

struct NRTHPSSParams
{
  std::shared_ptr<const BufferAdaptor> source;        // "source"
  index                                startFrame{0}; // Min(0)
  index                                numFrames{-1};
  index                                startChan{0};  // Min(0)
  index                                numChans{-1};
  std::shared_ptr<BufferAdaptor>       harmonic;      // "harmonic"
  std::shared_ptr<BufferAdaptor>       percussive;    // "percussive"
  std::shared_ptr<BufferAdaptor>       residual;      // "residual"
  index                                harmFilterSize{17}; // Odd, Min(3)
  index                                percFilterSize{31}; // Odd, Min(3)
  index                                maskingMode{0};     // Classic, Coupled, Advanced
  FloatPairsArray                      harmThresh;
  FloatPairsArray                      percThresh;
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
    outOnly(harmonic); // resized, every sample written
    outOnly(percussive);
    outOnly(residual);
  }
  void constrain()
  {
    startFrame = std::max<index>(0, startFrame);
    startChan = std::max<index>(0, startChan);
    impl::constrainFFT(fftSettings);
    harmFilterSize = detail::constrainFilterSize(harmFilterSize);
    percFilterSize = detail::constrainFilterSize(percFilterSize);
    maskingMode = std::min<index>(2, std::max<index>(0, maskingMode));
    harmThresh.constrain();
    percThresh.constrain();
  }
};
} // namespace hpss

class NRTHPSSClient
{
public:
  using ParamSetViewType = hpss::NRTHPSSParams;
  static constexpr ParamDescriptorList getParameterDescriptors() { return paramdesc::list(paramdesc::kBufHPSS); }

  NRTHPSSClient(ParamSetViewType& p, FluidContext&) : mParams(&p) {}
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
    BufferAdaptor* outputs[3] = {P.harmonic.get(), P.percussive.get(), P.residual.get()};
    bool           any = false;
    for (BufferAdaptor*& b : outputs)
    {
      if (b && !BufferAdaptor::Access(b).exists()) b = nullptr; // :333-346
      any = any || b != nullptr;
    }
    if (!any) return {S::kError, "No valid output has been set"};

    Result dev = mDevice.ensure(c.device());
    if (!dev.ok()) return dev;

    BufferAdaptor::ReadAccess source(P.source.get());
    const double              sampleRate = source.sampleRate();
    std::vector<float>        audio((size_t) (nChans * nFrames));
    for (index i = 0; i < nChans; ++i) // :499-509
      VectorView<float>(audio.data() + i * nFrames, nFrames) <<= source.samps(P.startFrame, nFrames, P.startChan + i);
    if (c.task() && !c.task()->iterationUpdate(0.0, 1.0)) return {S::kCancelled, ""};

    const FFTParams    f = P.fftSettings;
    const double       ht[4] = {P.harmThresh.value[0].first, P.harmThresh.value[0].second, P.harmThresh.value[1].first,
                                P.harmThresh.value[1].second};
    const double       pt[4] = {P.percThresh.value[0].first, P.percThresh.value[0].second, P.percThresh.value[1].first,
                                P.percThresh.value[1].second};
    std::vector<float> out((size_t) (nChans * 3 * nFrames));
    const int rc = fluhip_bufhpss_f32(mDevice.get(), audio.data(), nChans, nFrames, f.winSize(), f.fftSize(), f.hopSize(),
                                      P.harmFilterSize, P.percFilterSize, (int) P.maskingMode, ht, pt, out.data());
    if (rc != FLUHIP_OK) return mDevice.result(rc);
    if (FluidTask* task = c.task())
      if (!task->processUpdate(1.0, 1.0)) return {S::kCancelled, ""};

    for (int o = 0; o < 3; ++o) // :536-544
    {
      if (!outputs[o]) continue;
      BufferAdaptor::Access thisOutput(outputs[o]);
      Result                r = thisOutput.resize(nFrames, nChans, sampleRate);
      if (!r.ok()) return r;
      for (index j = 0; j < nChans; ++j)
        thisOutput.samps(j) <<= VectorView<const float>(out.data() + (j * 3 + o) * nFrames, nFrames);
    }
    return {};
  }

private:
  ParamSetViewType* mParams;
  DeviceContext     mDevice;
};

using NRTThreadedHPSSClient = NRTThreadingAdaptor<NRTHPSSClient>; // rt/HPSSClient.hpp:136

} // namespace fluhip
