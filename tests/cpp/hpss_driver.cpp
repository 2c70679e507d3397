// hpss_driver.cpp -- exercises the host-side BufHPSS client (include/flucoma_hip/HPSSClient.hpp) the way a host wrapper
// would.  Driven by tests/test_hpss_ref.py (CPU modes) and tests/test_gpu_hpss.py (run).
//
//   hpss_driver descriptors     the parameter table, in the format of client_driver descriptors
//   hpss_driver errors          the validation branches that need no device
//   hpss_driver constrain <hSize> <vSize> <mode> <hx1> <hy1> <hx2> <hy2> <win> <hop> <fft>
//   hpss_driver run <in.f32> <frames> <chans> <rate> <hSize> <vSize> <mode> <hx1> <hy1> <hx2> <hy2> <px1> <py1> <px2> <py2>
//                   <win> <hop> <fft> <withResidual> <async> <out.f32>
//       prints the status line and one shape line per output buffer; out.f32 receives the harmonic, the percussive and (when
//       it was given) the residual buffer, channel after channel
#include "../../include/flucoma_hip/HPSSClient.hpp"

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
  constexpr auto     list = fluhip::NRTThreadedHPSSClient::getParameterDescriptors();
  static const char* kinds[] = {"InputBuffer", "Buffer", "Long", "Float", "Enum", "FFT", "FloatPairsArray"};
  std::printf("{\n\"BufHPSS\": [");
  for (std::size_t i = 0; i < list.size(); i++)
  {
    const fluhip::ParamDescriptor& d = list[i];
    std::printf("%s{\"name\": \"%s\", \"display\": \"%s\", \"kind\": \"%s\"", i ? ", " : "", d.name, d.displayName,
                kinds[static_cast<int>(d.kind)]);
    if (d.kind == fluhip::ParamKind::kLong || d.kind == fluhip::ParamKind::kFloat || d.kind == fluhip::ParamKind::kEnum)
      std::printf(", \"default\": %.17g", d.defaultValue);
    if (d.kind == fluhip::ParamKind::kFFT) std::printf(", \"default\": [%ld, %ld, %ld]", (long) d.defaultValue, d.fftHop, d.fftSize);
    if (d.kind == fluhip::ParamKind::kFloatPairsArray)
    {
      std::printf(", \"default\": [");
      for (int j = 0; j < d.fixedSize; j++) std::printf("%s%.17g", j ? ", " : "", d.pairsDefault[j]);
      std::printf("], \"fixedSize\": %d", d.fixedSize);
    }
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
  std::printf("]\n}\n");
}

static int runErrors()
{
  FluidContext                ctx;
  fluhip::hpss::NRTHPSSParams p;
  fluhip::NRTHPSSClient       client(p, ctx);
  report("no_source", client.process<float>(ctx));
  p.source = makeBuffer(1, 4096);
  report("no_output", client.process<float>(ctx));
  p.residual = makeBuffer(1, 1);
  p.startFrame = 5000;
  report("start_past_end", client.process<float>(ctx));
  p.startFrame = 0;
  p.startChan = 3;
  report("chan_past_end", client.process<float>(ctx));
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
  if (mode == "errors") return runErrors();
  if (mode == "constrain")
  {
    if (argc < 12) return 2;
    fluhip::hpss::NRTHPSSParams p;
    p.harmFilterSize = std::atol(argv[2]);
    p.percFilterSize = std::atol(argv[3]);
    p.maskingMode = std::atol(argv[4]);
    p.harmThresh.value = {{{std::atof(argv[5]), std::atof(argv[6])}, {std::atof(argv[7]), std::atof(argv[8])}}};
    p.fftSettings = FFTParams(std::atol(argv[9]), std::atol(argv[10]), std::atol(argv[11]));
    p.constrain();
    std::printf("%ld %ld %ld %g %g %g %g %ld %ld %ld\n", (long) p.harmFilterSize, (long) p.percFilterSize, (long) p.maskingMode,
                p.harmThresh.value[0].first, p.harmThresh.value[0].second, p.harmThresh.value[1].first, p.harmThresh.value[1].second,
                (long) p.fftSettings.winSize(), (long) p.fftSettings.hopSize(), (long) p.fftSettings.fftSize());
    return 0;
  }
  if (mode == "run")
  {
    if (argc < 23) return 2;
    auto                        in = readFile(argv[2]);
    const idx                   frames = std::atol(argv[3]), chans = std::atol(argv[4]);
    fluhip::hpss::NRTHPSSParams p;
    p.source = makeBuffer(chans, frames, std::atof(argv[5]), in.data());
    p.harmFilterSize = std::atol(argv[6]);
    p.percFilterSize = std::atol(argv[7]);
    p.maskingMode = std::atol(argv[8]);
    p.harmThresh.value = {{{std::atof(argv[9]), std::atof(argv[10])}, {std::atof(argv[11]), std::atof(argv[12])}}};
    p.percThresh.value = {{{std::atof(argv[13]), std::atof(argv[14])}, {std::atof(argv[15]), std::atof(argv[16])}}};
    p.fftSettings = FFTParams(std::atol(argv[17]), std::atol(argv[18]), std::atol(argv[19]));
    const bool withResidual = std::atoi(argv[20]) != 0;
    std::shared_ptr<MemoryBufferAdaptor> outs[3] = {makeBuffer(3, 7), makeBuffer(3, 7), withResidual ? makeBuffer(3, 7) : nullptr};
    p.harmonic = outs[0];
    p.percussive = outs[1];
    p.residual = outs[2];
    // (no constrain(): the announced errors of the library must come back through the client)
    report("run", runJob<fluhip::NRTThreadedHPSSClient>(p, std::atoi(argv[21]) != 0));
    static const char* names[3] = {"harmonic", "percussive", "residual"};
    std::ofstream      f(argv[22], std::ios::binary);
    for (int o = 0; o < 3; o++)
    {
      if (!outs[o]) { std::printf("shape|%s|absent\n", names[o]); continue; }
      BufferAdaptor::ReadAccess a(outs[o].get());
      std::printf("shape|%s|%ld|%ld|%.17g\n", names[o], (long) a.numFrames(), (long) a.numChans(), a.sampleRate());
      for (idx c = 0; c < a.numChans(); ++c)
      {
        auto v = a.samps(c);
        for (idx i = 0; i < v.size(); ++i) { float x = v(i); f.write(reinterpret_cast<const char*>(&x), 4); }
      }
    }
    return 0;
  }
  return 2;
}
