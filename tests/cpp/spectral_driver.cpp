// spectral_driver.cpp -- exercises the host-side BufSpectralShape and BufChroma clients (include/flucoma_hip/SpectralShapeClient.hpp,
// ChromaClient.hpp) the way a host wrapper would.  Driven by tests/test_spectral_ref.py (CPU modes) and
// tests/test_gpu_spectral.py (run).
//
//   spectral_driver descriptors     the two parameter tables, in the format of client_driver descriptors
//   spectral_driver errors          the validation branches that need no device
//   spectral_driver defaults
//   spectral_driver constrain shape <select> <minFreq> <maxFreq> <rolloffPercent> <unit> <power> <win> <hop> <fft>
//   spectral_driver constrain chroma <numChroma> <ref> <normalize> <minFreq> <maxFreq> <win> <hop> <fft>
//   spectral_driver run shape <in.f32> <frames> <chans> <rate> <the nine of constrain shape> <padding> <async> <out.f32>
//   spectral_driver run chroma <in.f32> <frames> <chans> <rate> <the eight of constrain chroma> <padding> <async> <out.f32>
//       prints the status line and the shape line of the features buffer; out.f32 receives it channel after channel
#include "../../include/flucoma_hip/ChromaClient.hpp"
#include "../../include/flucoma_hip/SpectralShapeClient.hpp"

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
using ShapeParams = fluhip::spectralshape::NRTSpectralShapeParams;
using ChromaParams = fluhip::chroma::NRTChromaParams;

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

static void printTable(const char* name, const fluhip::ParamDescriptorList& list)
{
  static const char* kinds[] = {"InputBuffer", "Buffer", "Long", "Float", "Enum", "FFT", "FloatPairsArray", "Choices"};
  std::printf("\"%s\": [", name);
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
  std::printf("]");
}

static void printDescriptors()
{
  std::printf("{\n");
  printTable("BufSpectralShape", fluhip::NRTThreadedSpectralShapeClient::getParameterDescriptors());
  std::printf(",\n");
  printTable("BufChroma", fluhip::NRTThreadedChromaClient::getParameterDescriptors());
  std::printf("\n}\n");
}

template <class Client, class Params>
static void runErrors(const std::string& tag)
{
  FluidContext ctx;
  Params       p;
  Client       client(p, ctx);
  report(tag + "no_source", client.template process<float>(ctx));
  p.source = makeBuffer(1, 4096);
  report(tag + "no_output", client.template process<float>(ctx));
  p.features = makeBuffer(1, 1);
  p.startFrame = 5000;
  report(tag + "start_past_end", client.template process<float>(ctx));
  p.startFrame = 0;
  p.startChan = 3;
  report(tag + "chan_past_end", client.template process<float>(ctx));
}

static int setParams(ShapeParams& p, char** a)
{
  p.select = std::atol(a[0]);
  p.minFreq = std::atof(a[1]);
  p.maxFreq = std::atof(a[2]);
  p.rolloffPercent = std::atof(a[3]);
  p.unit = std::atol(a[4]);
  p.power = std::atol(a[5]);
  p.fftSettings = FFTParams(std::atol(a[6]), std::atol(a[7]), std::atol(a[8]));
  return 9;
}

static int setParams(ChromaParams& p, char** a)
{
  p.numChroma = std::atol(a[0]);
  p.ref = std::atof(a[1]);
  p.normalize = std::atol(a[2]);
  p.minFreq = std::atof(a[3]);
  p.maxFreq = std::atof(a[4]);
  p.fftSettings = FFTParams(std::atol(a[5]), std::atol(a[6]), std::atol(a[7]));
  return 8;
}

static void print(const ShapeParams& p, bool padding)
{
  std::printf("%ld %g %g %g %ld %ld %ld %ld %ld", (long) p.select, p.minFreq, p.maxFreq, p.rolloffPercent, (long) p.unit,
              (long) p.power, (long) p.fftSettings.winSize(), (long) p.fftSettings.hopSize(), (long) p.fftSettings.fftSize());
  if (padding) std::printf(" %ld", (long) p.padding);
  std::printf("\n");
}

static void print(const ChromaParams& p, bool padding)
{
  std::printf("%ld %g %ld %g %g %ld %ld %ld", (long) p.numChroma, p.ref, (long) p.normalize, p.minFreq, p.maxFreq,
              (long) p.fftSettings.winSize(), (long) p.fftSettings.hopSize(), (long) p.fftSettings.fftSize());
  if (padding) std::printf(" %ld", (long) p.padding);
  std::printf("\n");
}

// argv: <in.f32> <frames> <chans> <rate> <parameters> <padding> <async> <out.f32>
template <class Adaptor, class Params>
static int run(int argc, char** argv)
{
  Params    p;
  const int np = setParams(p, argv + 4); // (main has counted the arguments)
  if (argc < 4 + np + 3) return 2;
  auto      in = readFile(argv[0]);
  const idx frames = std::atol(argv[1]), chans = std::atol(argv[2]);
  p.source = makeBuffer(chans, frames, std::atof(argv[3]), in.data());
  p.padding = std::atol(argv[4 + np]);
  auto out = makeBuffer(3, 7);
  p.features = out;
  // (no constrain(): the announced errors of the library must come back through the client)
  report("run", runJob<Adaptor>(p, std::atoi(argv[5 + np]) != 0));
  std::ofstream             f(argv[6 + np], std::ios::binary);
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
    runErrors<fluhip::NRTSpectralShapeClient, ShapeParams>("shape_");
    runErrors<fluhip::NRTChromaClient, ChromaParams>("chroma_");
    return 0;
  }
  if (mode == "defaults")
  {
    std::printf("shape ");
    print(ShapeParams(), true);
    std::printf("chroma ");
    print(ChromaParams(), true);
    return 0;
  }
  if (argc < 3) return 2;
  const bool shape = std::string(argv[2]) == "shape";
  if (!shape && std::string(argv[2]) != "chroma") return 2;
  if (mode == "constrain")
  {
    if (argc < 3 + (shape ? 9 : 8)) return 2;
    if (shape)
    {
      ShapeParams p;
      setParams(p, argv + 3);
      p.constrain();
      print(p, false);
    }
    else
    {
      ChromaParams p;
      setParams(p, argv + 3);
      p.constrain();
      print(p, false);
    }
    return 0;
  }
  if (mode == "run")
  {
    if (argc < 3 + 4 + (shape ? 9 : 8) + 3) return 2;
    return shape ? run<fluhip::NRTThreadedSpectralShapeClient, ShapeParams>(argc - 3, argv + 3)
                 : run<fluhip::NRTThreadedChromaClient, ChromaParams>(argc - 3, argv + 3);
  }
  return 2;
}
