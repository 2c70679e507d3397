// loudness_driver.cpp -- exercises the host-side BufLoudness client (include/flucoma_hip/LoudnessClient.hpp) the way a host
// wrapper would.  Driven by tests/test_loudness_ref.py (CPU modes) and tests/test_gpu_loudness.py (run).
//
//   loudness_driver descriptors     the parameter table, in the format of client_driver descriptors (plus "fixed")
//   loudness_driver errors          the validation branches that need no device
//   loudness_driver defaults
//   loudness_driver constrain <select> <kWeighting> <truePeak> <windowSize> <hopSize> <maxWindowSize>
//   loudness_driver run <in.f32> <frames> <chans> <rate> <the six of constrain> <padding> <async> <out.f32>
//       prints the status line and the shape line of the features buffer; out.f32 receives it channel after channel
#include "../../include/flucoma_hip/LoudnessClient.hpp"

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
using Params = fluhip::loudness::NRTLoudnessParams;

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

static void report(const std::string& tag, const Result& r) { std::printf("%s|%d|%s\n", tag.c_str(), (int) r.status(), r.message().c_str()); }

// `interleaved`: frames x chans floats
static std::shared_ptr<MemoryBufferAdaptor> makeBuffer(idx chans, idx frames, double sr = 44100.0, const float* interleaved = nullptr)
{
  auto b = std::make_shared<MemoryBufferAdaptor>(chans, frames, sr);
  if (interleaved) std::memcpy(b->raw(), interleaved, sizeof(float) * (size_t) (chans * frames));
  return b;
}

static Result runJob(Params& p, bool async)
{
  fluhip::NRTThreadedLoudnessClient adaptor(p);
  Result                            r;
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

static void printDescriptors()
{
  static const char* kinds[] = {"InputBuffer", "Buffer", "Long", "Float", "Enum", "FFT", "FloatPairsArray", "Choices"};
  const fluhip::ParamDescriptorList list = fluhip::NRTThreadedLoudnessClient::getParameterDescriptors();
  std::printf("{\n\"BufLoudness\": [");
  for (std::size_t i = 0; i < list.size(); i++)
  {
    const fluhip::ParamDescriptor& d = list[i];
    const bool                     strings = d.kind == fluhip::ParamKind::kEnum || d.kind == fluhip::ParamKind::kChoices;
    std::printf("%s{\"name\": \"%s\", \"display\": \"%s\", \"kind\": \"%s\"", i ? ", " : "", d.name, d.displayName,
                kinds[static_cast<int>(d.kind)]);
    if (d.kind == fluhip::ParamKind::kLong || d.kind == fluhip::ParamKind::kFloat || strings)
      std::printf(", \"default\": %.17g", d.defaultValue);
    if (!strings && d.hasMin) std::printf(", \"min\": %.17g", d.min);
    if (!strings && d.hasMax) std::printf(", \"max\": %.17g", d.max);
    if (strings)
    {
      std::printf(", \"strings\": [");
      for (int j = 0; j < d.numEnumStrings; j++) std::printf("%s\"%s\"", j ? ", " : "", d.enumStrings[j]);
      std::printf("]");
    }
    if (d.relational) std::printf(", \"relational\": \"%s\"", d.relational);
    if (d.fixed) std::printf(", \"fixed\": true");
    std::printf("}");
  }
  std::printf("]\n}\n");
}

static void runErrors()
{
  FluidContext              ctx;
  Params                    p;
  fluhip::NRTLoudnessClient client(p, ctx);
  report("no_source", client.process<float>(ctx));
  p.source = makeBuffer(1, 4096);
  report("no_output", client.process<float>(ctx));
  p.features = makeBuffer(1, 1);
  p.startFrame = 5000;
  report("start_past_end", client.process<float>(ctx));
  p.startFrame = 0;
  p.startChan = 3;
  report("chan_past_end", client.process<float>(ctx));
  p.startChan = 0;
  // the parameter set's own bounds: announced in front of the device
  p.hopSize = 0;
  report("hop_zero", client.process<float>(ctx));
  p.hopSize = 512;
  p.windowSize = 0;
  report("window_zero", client.process<float>(ctx));
  p.windowSize = 16385;
  report("window_above_max", client.process<float>(ctx));
  p.windowSize = 1024;
  p.maxWindowSize = 3000;
  report("max_window_not_a_power_of_two", client.process<float>(ctx));
  p.maxWindowSize = 65536;
  report("max_window_too_large", client.process<float>(ctx));
}

static void setParams(Params& p, char** a)
{
  p.select = std::atol(a[0]);
  p.kWeighting = std::atol(a[1]);
  p.truePeak = std::atol(a[2]);
  p.windowSize = std::atol(a[3]);
  p.hopSize = std::atol(a[4]);
  p.maxWindowSize = std::atol(a[5]);
}

static void print(const Params& p, bool padding)
{
  std::printf("%ld %ld %ld %ld %ld %ld", (long) p.select, (long) p.kWeighting, (long) p.truePeak, (long) p.windowSize,
              (long) p.hopSize, (long) p.maxWindowSize);
  if (padding) std::printf(" %ld", (long) p.padding);
  std::printf("\n");
}

// argv: <in.f32> <frames> <chans> <rate> <six parameters> <padding> <async> <out.f32>
static int run(char** argv)
{
  Params p;
  setParams(p, argv + 4);
  auto      in = readFile(argv[0]);
  const idx frames = std::atol(argv[1]), chans = std::atol(argv[2]);
  p.source = makeBuffer(chans, frames, std::atof(argv[3]), in.data());
  p.padding = std::atol(argv[10]);
  auto out = makeBuffer(3, 7);
  p.features = out;
  // (no constrain(): the announced errors of the library must come back through the client)
  report("run", runJob(p, std::atoi(argv[11]) != 0));
  std::ofstream             f(argv[12], std::ios::binary);
  BufferAdaptor::ReadAccess a(out.get());
  std::printf("shape|features|%ld|%ld|%.17g\n", (long) a.numFrames(), (long) a.numChans(), a.sampleRate());
  for (idx c = 0; c < a.numChans(); ++c)
  {
    auto v = a.samps(c);
    for (idx i = 0; i < v.size(); ++i) { float x = v(i); f.write(reinterpret_cast<const char*>(&x), 4); }
  }
  return 0;
}

int main(int argc, char** argv)
{
  if (argc < 2) return 2;
  const std::string mode = argv[1];
  if (mode == "descriptors")
  {
    printDescriptors();
    return 0;
  }
  if (mode == "errors")
  {
    runErrors();
    return 0;
  }
  if (mode == "defaults")
  {
    print(Params(), true);
    return 0;
  }
  if (mode == "constrain")
  {
    if (argc < 2 + 6) return 2;
    Params p;
    setParams(p, argv + 2);
    p.constrain();
    print(p, false);
    return 0;
  }
  if (mode == "run")
  {
    if (argc < 2 + 13) return 2;
    return run(argv + 2);
  }
  return 2;
}
