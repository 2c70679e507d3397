// nmfcross_driver.cpp -- exercises the host-side BufNMFCross client (include/flucoma_hip/NMFCrossClient.hpp) the way a host
// wrapper would: MemoryBufferAdaptor buffers, NMFCrossParams, NRTNMFCrossClient sync / async.  Driven by
// tests/test_nmfcross_ref.py (CPU modes) and tests/test_gpu_nmfcross.py (run).
//
//   nmfcross_driver descriptors                the parameter table, in the format of client_driver descriptors
//   nmfcross_driver errors                     the validation branches that need no device (nrt/NMFCrossClient.hpp:94-118)
//   nmfcross_driver constrain <r> <p> <c> <iters> <win> <hop> <fft>   the constrained values
//   nmfcross_driver run <src.f32> <nsrc> <srcChans> <srcRate> <tgt.f32> <ntgt> <tgtChans> <tgtRate> <win> <hop> <fft>
//                       <r> <p> <c> <iters> <seed> <async> <out.bin>
#include "../../include/flucoma_hip/NMFCrossClient.hpp"

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
namespace nmfcross = fluhip::nmfcross;

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

// header {frames, chans} int64, sample rate double, then the channels one after the other as floats
static void writeBuffer(const std::string& path, const std::shared_ptr<MemoryBufferAdaptor>& b)
{
  BufferAdaptor::ReadAccess a(b.get());
  std::ofstream f(path, std::ios::binary);
  int64_t hdr[2] = {a.numFrames(), a.numChans()};
  double  sr = a.sampleRate();
  f.write(reinterpret_cast<const char*>(hdr), sizeof(hdr));
  f.write(reinterpret_cast<const char*>(&sr), sizeof(sr));
  for (idx c = 0; c < a.numChans(); ++c)
  {
    auto v = a.samps(c);
    for (idx i = 0; i < v.size(); ++i) { float x = v(i); f.write(reinterpret_cast<const char*>(&x), 4); }
  }
}

static void report(const char* tag, const Result& r) { std::printf("%s|%d|%s\n", tag, (int) r.status(), r.message().c_str()); }

static std::shared_ptr<MemoryBufferAdaptor> makeBuffer(idx chans, idx frames, double sr = 44100.0, const float* interleaved = nullptr)
{
  auto b = std::make_shared<MemoryBufferAdaptor>(chans, frames, sr);
  if (interleaved) std::memcpy(b->raw(), interleaved, sizeof(float) * (size_t) (chans * frames));
  return b;
}

static Result runJob(nmfcross::NMFCrossParams& p, bool async)
{
  fluhip::NRTNMFCrossClient adaptor(p);
  Result                    r;
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
  constexpr auto     list = fluhip::NRTNMFCrossClient::getParameterDescriptors();
  static const char* kinds[] = {"InputBuffer", "Buffer", "Long", "Float", "Enum", "FFT"};
  std::printf("{\n\"BufNMFCross\": [");
  for (std::size_t i = 0; i < list.size(); i++)
  {
    const fluhip::ParamDescriptor& d = list[i];
    std::printf("%s{\"name\": \"%s\", \"display\": \"%s\", \"kind\": \"%s\"", i ? ", " : "", d.name, d.displayName,
                kinds[static_cast<int>(d.kind)]);
    if (d.kind == fluhip::ParamKind::kLong || d.kind == fluhip::ParamKind::kFloat) std::printf(", \"default\": %.17g", d.defaultValue);
    if (d.kind == fluhip::ParamKind::kFFT) std::printf(", \"default\": [%ld, %ld, %ld]", (long) d.defaultValue, d.fftHop, d.fftSize);
    if (d.hasMin) std::printf(", \"min\": %.17g", d.min);
    if (d.hasMax) std::printf(", \"max\": %.17g", d.max);
    if (d.relational) std::printf(", \"relational\": \"%s\"", d.relational);
    std::printf("}");
  }
  std::printf("]\n}\n");
}

static int runErrors()
{
  FluidContext             ctx;
  nmfcross::NMFCrossParams p;
  nmfcross::NMFCrossClient client(p, ctx);
  report("no_source", client.process<float>(ctx));
  p.source = makeBuffer(1, 4096);
  report("no_target", client.process<float>(ctx));
  p.target = makeBuffer(1, 4096);
  report("no_output", client.process<float>(ctx));
  p.output = makeBuffer(1, 1);
  p.source = makeBuffer(1, 0);
  report("empty_source", client.process<float>(ctx));
  p.source = makeBuffer(1, 4096);
  p.target = makeBuffer(1, 0);
  report("empty_target", client.process<float>(ctx));
  p.target = makeBuffer(1, 1000);         // (1000 + 512) / 512 = 2 target frames
  report("sparsity_too_large", client.process<float>(ctx));
  p.timeSparsity = 1;
  report("continuity_too_large", client.process<float>(ctx));
  return 0;
}

int main(int argc, char** argv)
{
  if (argc < 2) return 2;
  const std::string mode = argv[1];
  if (mode == "descriptors") { printDescriptors(); return 0; }
  if (mode == "errors") return runErrors();
  if (mode == "constrain")
  {
    if (argc < 9) return 2;
    nmfcross::NMFCrossParams p;
    p.timeSparsity = std::atol(argv[2]);
    p.polyphony = std::atol(argv[3]);
    p.continuity = std::atol(argv[4]);
    p.iterations = std::atol(argv[5]);
    p.fftSettings = FFTParams(std::atol(argv[6]), std::atol(argv[7]), std::atol(argv[8]));
    p.constrain();
    std::printf("%ld %ld %ld %ld\n", (long) p.timeSparsity, (long) p.polyphony, (long) p.continuity, (long) p.iterations);
    return 0;
  }
  if (mode == "run")
  {
    if (argc < 20) return 2;
    auto          src = readFile(argv[2]);
    const idx     nsrc = std::atol(argv[3]), srcChans = std::atol(argv[4]);
    const double  srcRate = std::atof(argv[5]);
    auto          tgt = readFile(argv[6]);
    const idx     ntgt = std::atol(argv[7]), tgtChans = std::atol(argv[8]);
    const double  tgtRate = std::atof(argv[9]);
    nmfcross::NMFCrossParams p;
    p.source = makeBuffer(srcChans, nsrc, srcRate, src.data());
    p.target = makeBuffer(tgtChans, ntgt, tgtRate, tgt.data());
    auto out = makeBuffer(3, 7);
    p.output = out;
    p.fftSettings = FFTParams(std::atol(argv[10]), std::atol(argv[11]), std::atol(argv[12]));
    p.timeSparsity = std::atol(argv[13]);
    p.polyphony = std::atol(argv[14]);
    p.continuity = std::atol(argv[15]);
    p.iterations = std::atol(argv[16]);
    p.seed = std::atol(argv[17]);
    const bool async = std::atoi(argv[18]) != 0;
    p.constrain();
    report("run", runJob(p, async));
    writeBuffer(argv[19], out);
    return 0;
  }
  return 2;
}
