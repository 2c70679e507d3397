// amp_driver.cpp -- exercises the host-side BufAmpSlice / BufAmpFeature clients (include/flucoma_hip/AmpSliceClient.hpp,
// AmpFeatureClient.hpp) the way a host wrapper would.  Driven by tests/test_amp_ref.py (CPU modes) and tests/test_gpu_amp.py
// (slice / feature).
//
//   amp_driver descriptors     the two parameter tables, in the format of client_driver descriptors
//   amp_driver errors          the validation branches that need no device
//   amp_driver constrain <fastUp> <fastDown> <slowUp> <slowDown> <on> <off> <floor> <minSlice> <highPass>
//   amp_driver slice <in.f32> <frames> <chans> <rate> <startFrame> <fastUp> <fastDown> <slowUp> <slowDown> <on> <off> <floor>
//                    <minSlice> <highPass> <async>      prints status line, then the indices one per line
//   amp_driver feature <in.f32> <frames> <chans> <rate> <fastUp> <fastDown> <slowUp> <slowDown> <floor> <highPass> <out.f32>
#include "../../include/flucoma_hip/AmpFeatureClient.hpp"

#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>
#include <thread>

using fluhip::BufferAdaptor; using fluhip::FluidContext; using fluhip::MemoryBufferAdaptor;
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
    if (d.kind == fluhip::ParamKind::kLong || d.kind == fluhip::ParamKind::kFloat) std::printf(", \"default\": %.17g", d.defaultValue);
    if (d.hasMin) std::printf(", \"min\": %.17g", d.min);
    if (d.hasMax) std::printf(", \"max\": %.17g", d.max);
    if (d.relational) std::printf(", \"relational\": \"%s\"", d.relational);
    std::printf("}");
  }
  std::printf("]%s\n", last ? "" : ",");
}

static int runErrors()
{
  FluidContext ctx;
  {
    fluhip::ampslice::NRTAmpSliceParams p;
    fluhip::NRTAmpSliceClient           client(p, ctx);
    report("slice_no_source", client.process<float>(ctx));
    p.source = makeBuffer(1, 4096);
    report("slice_no_output", client.process<float>(ctx));
    p.indices = makeBuffer(1, 1);
    p.startFrame = 5000;
    report("slice_start_past_end", client.process<float>(ctx));
  }
  {
    fluhip::ampfeature::NRTAmpFeatureParams p;
    fluhip::NRTAmpFeatureClient             client(p, ctx);
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
    printDescriptors<fluhip::NRTAmpSliceClient>("BufAmpSlice", false);
    printDescriptors<fluhip::NRTAmpFeatureClient>("BufAmpFeature", true);
    std::printf("}\n");
    return 0;
  }
  if (mode == "errors") return runErrors();
  if (mode == "constrain")
  {
    if (argc < 11) return 2;
    fluhip::ampslice::NRTAmpSliceParams p;
    p.fastRampUp = std::atol(argv[2]);
    p.fastRampDown = std::atol(argv[3]);
    p.slowRampUp = std::atol(argv[4]);
    p.slowRampDown = std::atol(argv[5]);
    p.onThreshold = std::atof(argv[6]);
    p.offThreshold = std::atof(argv[7]);
    p.floor = std::atof(argv[8]);
    p.minSliceLength = std::atol(argv[9]);
    p.highPassFreq = std::atof(argv[10]);
    p.constrain();
    std::printf("%ld %ld %ld %ld %g %g %g %ld %g\n", (long) p.fastRampUp, (long) p.fastRampDown, (long) p.slowRampUp,
                (long) p.slowRampDown, p.onThreshold, p.offThreshold, p.floor, (long) p.minSliceLength, p.highPassFreq);
    return 0;
  }
  if (mode == "slice")
  {
    if (argc < 17) return 2;
    auto                                in = readFile(argv[2]);
    const idx                           frames = std::atol(argv[3]), chans = std::atol(argv[4]);
    fluhip::ampslice::NRTAmpSliceParams p;
    p.source = makeBuffer(chans, frames, std::atof(argv[5]), in.data());
    auto out = makeBuffer(3, 7);
    p.indices = out;
    p.startFrame = std::atol(argv[6]);
    p.fastRampUp = std::atol(argv[7]);
    p.fastRampDown = std::atol(argv[8]);
    p.slowRampUp = std::atol(argv[9]);
    p.slowRampDown = std::atol(argv[10]);
    p.onThreshold = std::atof(argv[11]);
    p.offThreshold = std::atof(argv[12]);
    p.floor = std::atof(argv[13]);
    p.minSliceLength = std::atol(argv[14]);
    p.highPassFreq = std::atof(argv[15]);
    p.constrain();
    report("run", runJob<fluhip::NRTThreadedAmpSliceClient>(p, std::atoi(argv[16]) != 0));
    BufferAdaptor::ReadAccess a(out.get());
    std::printf("shape|%ld|%ld|%.17g\n", (long) a.numFrames(), (long) a.numChans(), a.sampleRate());
    auto v = a.samps(0);
    for (idx i = 0; i < v.size(); ++i) std::printf("%ld\n", (long) v(i));
    return 0;
  }
  if (mode == "feature")
  {
    if (argc < 13) return 2;
    auto                                    in = readFile(argv[2]);
    const idx                               frames = std::atol(argv[3]), chans = std::atol(argv[4]);
    fluhip::ampfeature::NRTAmpFeatureParams p;
    p.source = makeBuffer(chans, frames, std::atof(argv[5]), in.data());
    auto out = makeBuffer(3, 7);
    p.features = out;
    p.fastRampUp = std::atol(argv[6]);
    p.fastRampDown = std::atol(argv[7]);
    p.slowRampUp = std::atol(argv[8]);
    p.slowRampDown = std::atol(argv[9]);
    p.floor = std::atof(argv[10]);
    p.highPassFreq = std::atof(argv[11]);
    p.constrain();
    report("run", runJob<fluhip::NRTThreadedAmpFeatureClient>(p, false));
    BufferAdaptor::ReadAccess a(out.get());
    std::printf("shape|%ld|%ld|%.17g\n", (long) a.numFrames(), (long) a.numChans(), a.sampleRate());
    std::ofstream f(argv[12], std::ios::binary);
    for (idx c = 0; c < a.numChans(); ++c)
    {
      auto v = a.samps(c);
      for (idx i = 0; i < v.size(); ++i) { float x = v(i); f.write(reinterpret_cast<const char*>(&x), 4); }
    }
    return 0;
  }
  return 2;
}
