// pitch_driver.cpp -- exercises the host-side BufPitch client (include/flucoma_hip/PitchClient.hpp) the way a host wrapper
// would.  Driven by tests/test_pitch_ref.py (CPU modes) and tests/test_gpu_pitch.py (run).
//
//   pitch_driver descriptors     the parameter table, in the format of client_driver descriptors
//   pitch_driver errors          the validation branches that need no device
//   pitch_driver constrain <select> <algorithm> <minFreq> <maxFreq> <unit> <win> <hop> <fft>
//   pitch_driver run <in.f32> <frames> <chans> <rate> <select> <algorithm> <minFreq> <maxFreq> <unit> <win> <hop> <fft>
//                    <padding> <async> <out.f32>
//       prints the status line and the shape line of the features buffer; out.f32 receives it channel after channel
#include "../../include/flucoma_hip/PitchClient.hpp"

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

static void printDescriptors()
{
  constexpr auto     list = fluhip::NRTThreadedPitchClient::getParameterDescriptors();
  static const char* kinds[] = {"InputBuffer", "Buffer", "Long", "Float", "Enum", "FFT", "FloatPairsArray", "Choices"};
  std::printf("{\n\"BufPitch\": [");
  for (std::size_t i = 0; i < list.size(); i++)
  {
    const fluhip::ParamDescriptor& d = list[i];
    const bool                     strings = d.kind == fluhip::ParamKind::kEnum || d.kind == fluhip::ParamKind::kChoices;
    std::printf("%s{\"name\": \"%s\", \"display\": \"%s\", \"kind\": \"%s\"", i ? ", " : "", d.name, d.displayName,
                kinds[static_cast<int>(d.kind)]);
    if (d.kind == fluhip::ParamKind::kLong || d.kind == fluhip::ParamKind::kFloat || strings)
      std::printf(", \"default\": %.17g", d.defaultValue);
    if (d.kind == fluhip::ParamKind::kFFT) std::printf(", \"default\": [%ld, %ld, %ld]", (long) d.defaultValue, d.fftHop, d.fftSize);
    if (!strings && d.hasMin) std::printf(", \"min\": %.17g", d.min);
    if (!strings && d.hasMax) std::printf(", \"max\": %.17g", d.max);
    if (strings)
    {
      std::printf(", \"strings\": [");
      for (int j = 0; j < d.numEnumStrings; j++) std::printf("%s\"%s\"", j ? ", " : "", d.enumStrings[j]);
      std::printf("]");
    }
    if (d.relational) std::printf(", \"relational\": \"%s\"", d.relational);
    std::printf("}");
  }
  std::printf("]\n}\n");
}

static int runErrors()
{
  FluidContext                  ctx;
  fluhip::pitch::NRTPitchParams p;
  fluhip::NRTPitchClient        client(p, ctx);
  report("no_source", client.process<float>(ctx));
  p.source = makeBuffer(1, 4096);
  report("no_output", client.process<float>(ctx));
  p.features = makeBuffer(1, 1);
  p.startFrame = 5000;
  report("start_past_end", client.process<float>(ctx));
  p.startFrame = 0;
  p.startChan = 3;
  report("chan_past_end", client.process<float>(ctx));
  return 0;
}

static void setParams(fluhip::pitch::NRTPitchParams& p, char** a)
{
  p.select = std::atol(a[0]);
  p.algorithm = std::atol(a[1]);
  p.minFreq = std::atof(a[2]);
  p.maxFreq = std::atof(a[3]);
  p.unit = std::atol(a[4]);
  p.fftSettings = FFTParams(std::atol(a[5]), std::atol(a[6]), std::atol(a[7]));
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
  if (mode == "errors") return runErrors();
  if (mode == "constrain")
  {
    if (argc < 10) return 2;
    fluhip::pitch::NRTPitchParams p;
    setParams(p, argv + 2);
    p.constrain();
    std::printf("%ld %ld %g %g %ld %ld %ld %ld\n", (long) p.select, (long) p.algorithm, p.minFreq, p.maxFreq, (long) p.unit,
                (long) p.fftSettings.winSize(), (long) p.fftSettings.hopSize(), (long) p.fftSettings.fftSize());
    return 0;
  }
  if (mode == "defaults")
  {
    fluhip::pitch::NRTPitchParams p;
    std::printf("%ld %ld %g %g %ld %ld %ld %ld %ld\n", (long) p.select, (long) p.algorithm, p.minFreq, p.maxFreq, (long) p.unit,
                (long) p.fftSettings.winSize(), (long) p.fftSettings.hopSize(), (long) p.fftSettings.fftSize(), (long) p.padding);
    return 0;
  }
  if (mode == "run")
  {
    if (argc < 17) return 2;
    auto                          in = readFile(argv[2]);
    const idx                     frames = std::atol(argv[3]), chans = std::atol(argv[4]);
    fluhip::pitch::NRTPitchParams p;
    p.source = makeBuffer(chans, frames, std::atof(argv[5]), in.data());
    setParams(p, argv + 6);
    p.padding = std::atol(argv[14]);
    auto out = makeBuffer(3, 7);
    p.features = out;
    // (no constrain(): the announced errors of the library must come back through the client)
    report("run", runJob<fluhip::NRTThreadedPitchClient>(p, std::atoi(argv[15]) != 0));
    std::ofstream             f(argv[16], std::ios::binary);
    BufferAdaptor::ReadAccess a(out.get());
    std::printf("shape|features|%ld|%ld|%.17g\n", (long) a.numFrames(), (long) a.numChans(), a.sampleRate());
    for (idx c = 0; c < a.numChans(); ++c)
    {
      auto v = a.samps(c);
      for (idx i = 0; i < v.size(); ++i) { float x = v(i); f.write(reinterpret_cast<const char*>(&x), 4); }
    }
    return 0;
  }
  return 2;
}
