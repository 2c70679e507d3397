// onset_driver.cpp -- exercises the host-side BufOnsetSlice / BufOnsetFeature clients
// (include/flucoma_hip/OnsetSliceClient.hpp) the way a host wrapper would.  Driven by tests/test_onset_ref.py (CPU modes)
// and tests/test_gpu_onset.py (slice / feature).
//
//   onset_driver descriptors     the two parameter tables, in the format of client_driver descriptors
//   onset_driver errors          the validation branches that need no device
//   onset_driver constrain <metric> <threshold> <minSlice> <filter> <frameDelta> <win> <hop> <fft>
//   onset_driver slice <in.f32> <frames> <chans> <rate> <startFrame> <metric> <threshold> <minSlice> <filter> <frameDelta>
//                      <win> <hop> <fft> <async>      prints status line, then the indices one per line
//   onset_driver feature <in.f32> <frames> <chans> <rate> <metric> <filter> <frameDelta> <win> <hop> <fft> <padding> <out.f32>
#include "../../include/flucoma_hip/OnsetSliceClient.hpp"

#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>
#include <thread>

using fluhip::BufferAdaptor; using fluhip::FFTParams; using fluhip::FluidContext; using fluhip::MemoryBufferAdaptor;
using fluhip::ProcessState; using fluhip::Result; using fluhip::kProcessing;
using idx = fluhip::index;

static std::vector<float> readFile(const char* path)
{
  std::ifstream f(path, std::ios::binary | std::ios::ate);
  if (!f) { std::fprintf(stderr, "cannot read %s\n", path); std::exit(3); }
  const size_t bytes = (size_t) f.tellg();
  f.seekg(0);
  std::vector<float> v(bytes / sizeof(float));
  f.read(reinterpret_cast<char*>(v.data()), (std::streamsize) bytes);
  return v;
}

static void report(const char* tag, const Result& r) { std::printf("%s|%d|%s\n", tag, (int) r.status(), r.message().c_str()); }

// `interleaved`: frames x chans floats
static std::shared_ptr<MemoryBufferAdaptor> makeBuffer(idx chans, idx frames, double sr = 44100.0, const float* interleaved = nullptr)
{
  auto b = std::make_shared<MemoryBufferAdaptor>(chans, frames, sr);
  if (interleaved) std::memcpy(b->raw(), interleaved, sizeof(float) * (size_t) (chans * frames));
  return b;
}

template <class Adaptor, class Params>
static Result runJob(Params& p, bool async)
{
  Adaptor adaptor(p);
  Result  r;
  adaptor.enqueue(p);
  if (!async)
  {
    adaptor.setSynchronous(true);
    return adaptor.process();
  }
  report("process", adaptor.process());
  ProcessState st = kProcessing;
  while (st == kProcessing)
  {
    st = adaptor.checkProgress(r);
    std::this_thread::sleep_for(std::chrono::milliseconds(1));
  }
  return r;
}

template <class Client>
static void printDescriptors(const char* client, bool last)
{
  constexpr auto     list = Client::getParameterDescriptors();
  static const char* kinds[] = {"InputBuffer", "Buffer", "Long", "Float", "Enum", "FFT"};
  std::printf("\"%s\": [", client);
  for (std::size_t i = 0; i < list.size(); i++)
  {
    const fluhip::ParamDescriptor& d = list[i];
    std::printf("%s{\"name\": \"%s\", \"display\": \"%s\", \"kind\": \"%s\"", i ? ", " : "", d.name, d.displayName,
                kinds[static_cast<int>(d.kind)]);
    if (d.kind == fluhip::ParamKind::kLong || d.kind == fluhip::ParamKind::kFloat || d.kind == fluhip::ParamKind::kEnum)
      std::printf(", \"default\": %.17g", d.defaultValue);
    if (d.kind == fluhip::ParamKind::kFFT) std::printf(", \"default\": [%ld, %ld, %ld]", (long) d.defaultValue, d.fftHop, d.fftSize);
    if (d.kind != fluhip::ParamKind::kEnum && d.hasMin) std::printf(", \"min\": %.17g", d.min);
    if (d.kind != fluhip::ParamKind::kEnum && d.hasMax) std::printf(", \"max\": %.17g", d.max);
    if (d.kind == fluhip::ParamKind::kEnum)
    {
      std::printf(", \"strings\": [");
      for (int j = 0; j < d.numEnumStrings; j++) std::printf("%s\"%s\"", j ? ", " : "", d.enumStrings[j]);
      std::printf("]");
    }
    if (d.relational) std::printf(", \"relational\": \"%s\"", d.relational);
    std::printf("}");
  }
  std::printf("]%s\n", last ? "" : ",");
}

static int runErrors()
{
  FluidContext ctx;
  {
    fluhip::onsetslice::NRTOnsetSliceParams p;
    fluhip::NRTOnsetSliceClient             client(p, ctx);
    report("slice_no_source", client.process<float>(ctx));
    p.source = makeBuffer(1, 4096);
    report("slice_no_output", client.process<float>(ctx));
    p.indices = makeBuffer(1, 1);
    p.startFrame = 5000;
    report("slice_start_past_end", client.process<float>(ctx));
  }
  {
    fluhip::onsetfeature::NRTOnsetFeatureParams p;
    fluhip::NRTOnsetFeatureClient               client(p, ctx);
    report("feature_no_source", client.process<float>(ctx));
    p.source = makeBuffer(1, 4096);
    report("feature_no_output", client.process<float>(ctx));
  }
  return 0;
}

int main(int argc, char** argv)
{
  if (argc < 2) return 2;
  const std::string mode = argv[1];
  if (mode == "descriptors")
  {
    std::printf("{\n");
    printDescriptors<fluhip::NRTOnsetSliceClient>("BufOnsetSlice", false);
    printDescriptors<fluhip::NRTOnsetFeatureClient>("BufOnsetFeature", true);
    std::printf("}\n");
    return 0;
  }
  if (mode == "errors") return runErrors();
  if (mode == "constrain")
  {
    if (argc < 10) return 2;
    fluhip::onsetslice::NRTOnsetSliceParams p;
    p.metric = std::atol(argv[2]);
    p.threshold = std::atof(argv[3]);
    p.minSliceLength = std::atol(argv[4]);
    p.filterSize = std::atol(argv[5]);
    p.frameDelta = std::atol(argv[6]);
    p.fftSettings = FFTParams(std::atol(argv[7]), std::atol(argv[8]), std::atol(argv[9]));
    p.constrain();
    std::printf("%ld %g %ld %ld %ld %ld %ld %ld\n", (long) p.metric, p.threshold, (long) p.minSliceLength, (long) p.filterSize,
                (long) p.frameDelta, (long) p.fftSettings.winSize(), (long) p.fftSettings.hopSize(), (long) p.fftSettings.fftSize());
    return 0;
  }
  if (mode == "slice")
  {
    if (argc < 16) return 2;
    auto                                    in = readFile(argv[2]);
    const idx                               frames = std::atol(argv[3]), chans = std::atol(argv[4]);
    fluhip::onsetslice::NRTOnsetSliceParams p;
    p.source = makeBuffer(chans, frames, std::atof(argv[5]), in.data());
    auto out = makeBuffer(3, 7);
    p.indices = out;
    p.startFrame = std::atol(argv[6]);
    p.metric = std::atol(argv[7]);
    p.threshold = std::atof(argv[8]);
    p.minSliceLength = std::atol(argv[9]);
    p.filterSize = std::atol(argv[10]);
    p.frameDelta = std::atol(argv[11]);
    p.fftSettings = FFTParams(std::atol(argv[12]), std::atol(argv[13]), std::atol(argv[14]));
    p.constrain();
    report("run", runJob<fluhip::NRTThreadingOnsetSliceClient>(p, std::atoi(argv[15]) != 0));
    BufferAdaptor::ReadAccess a(out.get());
    std::printf("shape|%ld|%ld|%.17g\n", (long) a.numFrames(), (long) a.numChans(), a.sampleRate());
    auto v = a.samps(0);
    for (idx i = 0; i < v.size(); ++i) std::printf("%ld\n", (long) v(i));
    return 0;
  }
  if (mode == "feature")
  {
    if (argc < 14) return 2;
    auto                                        in = readFile(argv[2]);
    const idx                                   frames = std::atol(argv[3]), chans = std::atol(argv[4]);
    fluhip::onsetfeature::NRTOnsetFeatureParams p;
    p.source = makeBuffer(chans, frames, std::atof(argv[5]), in.data());
    auto out = makeBuffer(3, 7);
    p.features = out;
    p.metric = std::atol(argv[6]);
    p.filterSize = std::atol(argv[7]);
    p.frameDelta = std::atol(argv[8]);
    p.fftSettings = FFTParams(std::atol(argv[9]), std::atol(argv[10]), std::atol(argv[11]));
    p.padding = std::atol(argv[12]);
    p.constrain();
    report("run", runJob<fluhip::NRTThreadedOnsetFeatureClient>(p, false));
    BufferAdaptor::ReadAccess a(out.get());
    std::printf("shape|%ld|%ld|%.17g\n", (long) a.numFrames(), (long) a.numChans(), a.sampleRate());
    std::ofstream f(argv[13], std::ios::binary);
    for (idx c = 0; c < a.numChans(); ++c)
    {
      auto v = a.samps(c);
      for (idx i = 0; i < v.size(); ++i) { float x = v(i); f.write(reinterpret_cast<const char*>(&x), 4); }
    }
    return 0;
  }
  return 2;
}
