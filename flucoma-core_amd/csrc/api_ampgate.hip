// api_ampgate.hip -- C ABI of BufAmpGate:
//   fluhip_amp_gate_f64       algorithm::EnvelopeGate::processSample   algorithms/public/EnvelopeGate.hpp:64-175
//   fluhip_bufampgate_f32     NRTAmpGateClient   clients/rt/AmpGateClient.hpp:135-188, common/SpikesToTimes.hpp
//   fluhip_debug_ampgate_plan
// The front end is K15's (launch_amp_level, fluhip_amp.h), with the gate's own floor; the kernels behind it are in
// kernels_ampgate.hip (fluhip_ampgate.h).  No event, no stream is taken.  The device buffers of a call are its own (GateBuf:
// hipMalloc, hipFree when the call ends) and do NOT go through the caching block pool: a gate call asks for blocks of many sizes
// (a plane and a record row per signal of n + latency samples, byte planes of n), and what it would leave in the cache is what a
// later call of another entry point is handed.  That mattered while the STFT gather loaded one sample outside its buffer for a
// frame that lay wholly outside it (closed: the gather's loads stay inside [0, n), frame_window.h) -- what the
// cache held then decided whether such a call faulted; a gate call leaves the cache exactly as it found it.  The form is kept
// as it is (undoing it changes allocation and timing and is a change of its own).  The price is one hipMalloc / hipFree per
// buffer and call, a millisecond or two of a call that runs two serial passes.
#include "api_internal.h"
#include "fluhip_amp.h"
#include "fluhip_ampgate.h"
#include "fluhip_novelty.h" // launch_mono_sum_f32

namespace {

constexpr int64_t kWorkCapBytes = (int64_t) 1 << 30; // 1 GiB of samples and workspace per round

// a device buffer of one call, outside the block pool (see the head of the file)
struct GateBuf
{
  void* p = nullptr;
  GateBuf() = default;
  GateBuf(const GateBuf&) = delete;
  GateBuf& operator=(const GateBuf&) = delete;
  ~GateBuf()
  {
    if (p) (void) hipFree(p); // (waits for the device: the call's launches are behind it)
  }
  hipError_t alloc(size_t n)
  {
    const hipError_t e = hipMalloc(&p, n ? n : 16);
    if (e != hipSuccess) p = nullptr;
    return e;
  }
  template <typename T> T* as() const { return static_cast<T*>(p); }
};

#define GATE_ALLOC(ctx, buf, bytes)                                                                          \
  do                                                                                                         \
  {                                                                                                          \
    hipError_t e__ = (buf).alloc((bytes));                                                                   \
    if (e__ != hipSuccess) return fail_hip((ctx), e__, "device allocation of the amp gate workspace");       \
  } while (0)

int failn(fluhip_ctx* ctx, const char* msg) { return ctx ? fail(ctx, msg) : (int) FLUHIP_ERROR; }

struct GateParams
{
  int64_t rampUp, rampDown;
  double on, off;
  int64_t minSlice, minSilence, minAbove, minBelow, lookBack, lookAhead, maxSize;
};

bool in_db_range(double v) { return v >= -144.0 && v <= 144.0; } // (false for NaN)

// the reference's parameter table (AmpGateClient.hpp:42-56) and EnvelopeGate::init's assertion (:49): what it would clamp or
// abort on is refused.  *latency: L
int check_gate_params(fluhip_ctx* ctx, const GateParams& a, int64_t* latency)
{
  if (a.rampUp < 1) return fail(ctx, "rampUp must be at least 1");
  if (a.rampDown < 1) return fail(ctx, "rampDown must be at least 1");
  if (!in_db_range(a.on)) return fail(ctx, "onThreshold must be in [-144, 144]");
  if (!in_db_range(a.off)) return fail(ctx, "offThreshold must be in [-144, 144]");
  if (a.minSlice < 1) return fail(ctx, "minSliceLength must be at least 1");
  if (a.minSilence < 1) return fail(ctx, "minSilenceLength must be at least 1");
  if (a.minAbove < 1) return fail(ctx, "minLengthAbove must be at least 1");
  if (a.minBelow < 1) return fail(ctx, "minLengthBelow must be at least 1");
  if (a.lookBack < 0) return fail(ctx, "lookBack must be >= 0");
  if (a.lookAhead < 0) return fail(ctx, "lookAhead must be >= 0");
  if (a.maxSize < 1) return fail(ctx, "maxSize must be at least 1");
  // (compared one by one first: the sum of two int64 may not exist)
  if (a.minAbove > a.maxSize || a.lookBack > a.maxSize - a.minAbove || a.minBelow > a.maxSize || a.lookAhead > a.maxSize)
    return fail(ctx, "the latency max(minLengthAbove + lookBack, max(minLengthBelow, lookAhead)) exceeds maxSize");
  *latency = std::max(a.minAbove + a.lookBack, std::max(a.minBelow, a.lookAhead));
  return FLUHIP_OK;
}

int check_hipass(fluhip_ctx* ctx, double hipass)
{
  if (!(hipass >= 0.0 && hipass <= 0.5)) return fail(ctx, "hipass (the cutoff as a fraction of the sample rate) must be in [0, 0.5]");
  return FLUHIP_OK;
}

// AmpGateClient::process :92: min(highPassFreq / sampleRate, 0.5)
int client_hipass(fluhip_ctx* ctx, double highPassFreq, double sampleRate, double* hipass)
{
  if (!(highPassFreq >= 0.0) || !std::isfinite(highPassFreq)) return fail(ctx, "highPassFreq must be finite and >= 0");
  if (!(sampleRate > 0.0) || !std::isfinite(sampleRate)) return fail(ctx, "sample rate must be positive and finite");
  *hipass = std::min(highPassFreq / sampleRate, 0.5);
  return FLUHIP_OK;
}

// `steps` is n, or n + L for the client
int check_shape(fluhip_ctx* ctx, int64_t count, int64_t channels, int64_t n, int64_t extra)
{
  if (count < 1) return fail(ctx, "count: need at least one buffer");
  if (channels < 1) return fail(ctx, "channels: need at least one channel");
  if (n < 1) return fail(ctx, "n: need at least one sample");
  const int64_t most = INT64_MAX / 64 / count / channels;
  if (n > most || extra > most - n) return fail(ctx, "batch too large");
  return FLUHIP_OK;
}

// what one call builds on the host, and the workspaces of its rounds
struct GateWork
{
  fluhip::AmpHighPass hp;
  fluhip::AmpTransition M;
  fluhip::AmpGate gate;
  GateBuf front, plane, records, nrec;
};

int gate_work_init(GateWork& w, fluhip_ctx* ctx, const GateParams& a, int64_t latency, double hipass, int64_t signals, int64_t steps)
{
  w.hp = fluhip::amp_highpass(hipass);
  if (w.hp.on) w.M = fluhip::amp_transition(w.hp);
  // SlideUDFilter::updateCoeffs :19-23
  w.gate.up = 1.0 / (double) a.rampUp;
  w.gate.down = 1.0 / (double) a.rampDown;
  w.gate.floorDb = std::min(a.on, a.off) - 1; // EnvelopeGate.hpp:52, :85
  w.gate.on = a.on;
  w.gate.off = a.off;
  w.gate.minSlice = a.minSlice;
  w.gate.minSilence = a.minSilence;
  w.gate.minAbove = a.minAbove;
  w.gate.minBelow = a.minBelow;
  w.gate.lookBack = a.lookBack;
  w.gate.lookAhead = a.lookAhead;
  w.gate.latency = latency;
  GATE_ALLOC(ctx, w.front, (size_t) (signals * fluhip::amp_front_doubles(steps)) * sizeof(double));
  GATE_ALLOC(ctx, w.plane, (size_t) (signals * steps) * sizeof(double));
  GATE_ALLOC(ctx, w.records, (size_t) (signals * steps) * sizeof(int64_t));
  GATE_ALLOC(ctx, w.nrec, (size_t) signals * sizeof(int64_t));
  return FLUHIP_OK;
}

// bytes of workspace a signal of `steps` samples takes in GateWork
int64_t gate_work_bytes(int64_t steps)
{
  return steps * (int64_t) (sizeof(double) + sizeof(int64_t)) + fluhip::amp_front_doubles(steps) * (int64_t) sizeof(double);
}

// the smoothed plane of the signals p stays in w.plane; out (device, nb x outN bytes): y[t + first - L] (launch_ampgate_paint)
int gate_round(GateWork& w, fluhip_ctx* ctx, const fluhip::AmpSignals& p, int64_t outN, int64_t first, unsigned char* out)
{
  hipStream_t s = ctx->stream;
  {
    ProfScope ps(ctx, 2); // (the feature kernels' class: one record per round, uploads and the copy back outside it)
    fluhip::launch_amp_level(p, w.hp, w.M, w.gate.floorDb, w.front.as<double>(), w.plane.as<double>(), s);
    fluhip::launch_ampgate_follow(w.plane.as<double>(), p.count, p.n, w.gate, s);
    fluhip::launch_ampgate_machine(w.plane.as<double>(), p.count, p.n, w.gate, w.records.as<int64_t>(), w.nrec.as<int64_t>(), s);
    fluhip::launch_ampgate_paint(w.records.as<int64_t>(), w.nrec.as<int64_t>(), p.count, p.n, outN, first, out, s);
  }
  HIPCHK(ctx, hipGetLastError());
  return FLUHIP_OK;
}

// signals a round holds: `perSignal` bytes of samples, workspace and results each within the cap, at least one; whole groups of
// the serial kernels' 64 when there are that many (a round is never cut inside a signal)
int64_t signals_per_round(int64_t signals, int64_t perSignal)
{
  int64_t nb = std::min(signals, std::max<int64_t>(1, kWorkCapBytes / perSignal));
  if (nb >= fluhip::kAmpGateSignals) nb -= nb % fluhip::kAmpGateSignals;
  return nb;
}

int amp_gate_impl(fluhip_ctx* ctx, const double* x, int64_t count, int64_t n, int64_t ld, const GateParams& a, double hipass,
                  unsigned char* out, double* smoothed)
{
  int64_t L = 0;
  int rc = check_gate_params(ctx, a, &L);
  if (rc) return rc;
  if ((rc = check_hipass(ctx, hipass))) return rc;
  if ((rc = check_shape(ctx, count, 1, n, 0))) return rc;
  if (!x || !out) return fail(ctx, "null buffer");
  if (ld < n) return fail(ctx, "signal stride below the number of samples");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  const int64_t perSignal = n * ((int64_t) sizeof(double) + 1) + gate_work_bytes(n);
  const int64_t perB = signals_per_round(count, perSignal);
  GateWork w;
  if ((rc = gate_work_init(w, ctx, a, L, hipass, perB, n))) return rc;
  GateBuf dX, dOut;
  GATE_ALLOC(ctx, dX, (size_t) (perB * n) * sizeof(double));
  GATE_ALLOC(ctx, dOut, (size_t) (perB * n));
  for (int64_t b0 = 0; b0 < count; b0 += perB)
  {
    const int64_t nb = std::min(perB, count - b0);
    HIPCHK(ctx, hipMemcpy2DAsync(dX.p, (size_t) n * sizeof(double), x + b0 * ld, (size_t) ld * sizeof(double),
                                 (size_t) n * sizeof(double), (size_t) nb, hipMemcpyDefault, s));
    const fluhip::AmpSignals p{nullptr, dX.as<double>(), n, nb, n};
    // processSample at step t returns y[t - L + 1]
    if ((rc = gate_round(w, ctx, p, n, 1, dOut.as<unsigned char>()))) return rc;
    HIPCHK(ctx, hipStreamSynchronize(s)); // nothing is written to the caller's buffers before the device work has succeeded
    const size_t bytes = (size_t) (nb * n) * sizeof(double);
    if (smoothed && (rc = copy_to_host(ctx, smoothed + b0 * n, bytes, w.plane.p, bytes, bytes, 1, s))) return rc;
    HIPCHK(ctx, hipMemcpyAsync(out + b0 * n, dOut.p, (size_t) (nb * n), hipMemcpyDeviceToHost, s));
    HIPCHK(ctx, hipStreamSynchronize(s));
  }
  return FLUHIP_OK;
}

// NRTAmpGate::process :168-182 + spikesToTimes on o[0 .. n - 1].  Returns the number of pairs, or -1 where the two rows
// differ in number (then nothing is written); a lone (-1, -1) when nothing switches.  At most `capacity` values per row
int64_t switch_points(const unsigned char* o, int64_t n, int64_t startFrame, int64_t* onsets, int64_t* offsets, int64_t capacity)
{
  // the two counts first: nothing may be written where they differ
  int64_t on = o[0] == 1 ? 1 : 0, off = o[n - 1] == 1 ? 1 : 0;
  for (int64_t i = 1; i < n - 1; i++)
  {
    if (o[i] == 1 && o[i - 1] == 0) on++;
    if (o[i] == 0 && o[i - 1] == 1) off++;
  }
  if (on != off) return -1;
  if (on == 0)
  {
    if (capacity > 0) onsets[0] = offsets[0] = -1;
    return 1;
  }
  int64_t a = 0, b = 0;
  auto put = [&](int64_t* row, int64_t& k, int64_t v) { if (k < capacity) row[k] = v + startFrame; k++; };
  if (o[0] == 1) put(onsets, a, 0);
  for (int64_t i = 1; i < n - 1; i++)
  {
    if (o[i] == 1 && o[i - 1] == 0) put(onsets, a, i);
    if (o[i] == 0 && o[i - 1] == 1) put(offsets, b, i);
  }
  if (o[n - 1] == 1) put(offsets, b, n - 1);
  return on;
}

int bufampgate_impl(fluhip_ctx* ctx, const float* audio, int64_t count, int64_t channels, int64_t n, int64_t startFrame,
                    const GateParams& a, double highPassFreq, double sampleRate, int64_t* indices, int64_t capacity, int64_t* counts)
{
  int64_t L = 0;
  int rc = check_gate_params(ctx, a, &L);
  if (rc) return rc;
  double hipass = 0;
  if ((rc = client_hipass(ctx, highPassFreq, sampleRate, &hipass))) return rc;
  if ((rc = check_shape(ctx, count, channels, n, L))) return rc;
  if (!audio || !counts || (!indices && capacity > 0)) return fail(ctx, "null buffer");
  if (capacity < 0) return fail(ctx, "negative capacity");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  // NRTAmpGate::process :146-165: the channels summed in float into n + L samples, a zero tail behind them
  const int64_t steps = n + L;
  const int64_t perSignal = n * (channels > 1 ? channels + 1 : 1) * (int64_t) sizeof(float) + steps * (int64_t) sizeof(float) + n +
                            gate_work_bytes(steps);
  const int64_t perB = signals_per_round(count, perSignal);
  GateWork w;
  if ((rc = gate_work_init(w, ctx, a, L, hipass, perB, steps))) return rc;
  GateBuf dIn, dMono, dPad, dOut;
  GATE_ALLOC(ctx, dIn, (size_t) (perB * channels * n) * sizeof(float));
  if (channels > 1) GATE_ALLOC(ctx, dMono, (size_t) (perB * n) * sizeof(float));
  GATE_ALLOC(ctx, dPad, (size_t) (perB * steps) * sizeof(float));
  GATE_ALLOC(ctx, dOut, (size_t) (perB * n));
  std::vector<unsigned char> o((size_t) (perB * n));
  bool told = false;
  for (int64_t b0 = 0; b0 < count; b0 += perB)
  {
    const int64_t nb = std::min(perB, count - b0);
    HIPCHK(ctx, hipMemcpyAsync(dIn.p, audio + b0 * channels * n, (size_t) (nb * channels * n) * sizeof(float), hipMemcpyDefault, s));
    const float* mono = dIn.as<float>();
    if (channels > 1)
    {
      fluhip::launch_mono_sum_f32(dIn.as<float>(), (int) channels, n, nb, dMono.as<float>(), s);
      mono = dMono.as<float>();
    }
    HIPCHK(ctx, hipMemsetAsync(dPad.p, 0, (size_t) (nb * steps) * sizeof(float), s));
    HIPCHK(ctx, hipMemcpy2DAsync(dPad.p, (size_t) steps * sizeof(float), mono, (size_t) n * sizeof(float), (size_t) n * sizeof(float),
                                 (size_t) nb, hipMemcpyDeviceToDevice, s));
    const fluhip::AmpSignals p{dPad.as<float>(), nullptr, steps, nb, steps};
    // o[i] = output[padding + i] = y[i + 1]
    if ((rc = gate_round(w, ctx, p, n, L + 1, dOut.as<unsigned char>()))) return rc;
    HIPCHK(ctx, hipMemcpyAsync(o.data(), dOut.p, (size_t) (nb * n), hipMemcpyDeviceToHost, s));
    HIPCHK(ctx, hipStreamSynchronize(s));
    for (int64_t b = 0; b < nb; b++)
    {
      int64_t* rows = indices ? indices + (b0 + b) * 2 * capacity : nullptr;
      counts[b0 + b] = switch_points(o.data() + b * n, n, startFrame, rows, rows ? rows + capacity : nullptr, capacity);
      if (counts[b0 + b] < 0 && !told)
      {
        told = true;
        ctx->err = "buffer " + std::to_string(b0 + b) + ": the gate changes on the last sample, onsets and offsets differ in number "
                   "(the reference asserts); its count is -1 and its indices are not written";
      }
    }
  }
  return FLUHIP_OK;
}

} // namespace

extern "C" {

int fluhip_debug_ampgate_plan(fluhip_ctx* ctx, int64_t* out4)
{
  if (!out4) return failn(ctx, "null buffer");
  out4[0] = fluhip::kAmpGateFormThreeLaunches;
  out4[1] = fluhip::kAmpGateSignals;
  out4[2] = fluhip::kAmpGateTile;
  out4[3] = 0; // a lookup reads its window from the finished plane in global memory
  return FLUHIP_OK;
}

int fluhip_amp_gate_f64(fluhip_ctx* ctx, const double* x, int64_t count, int64_t n, int64_t ld, int64_t ramp_up, int64_t ramp_down,
                        double on, double off, int64_t min_slice, int64_t min_silence, int64_t min_above, int64_t min_below,
                        int64_t look_back, int64_t look_ahead, double hipass, int64_t max_size, unsigned char* out, double* smoothed)
{
  return guarded(ctx, [&] {
    const GateParams a{ramp_up, ramp_down, on, off, min_slice, min_silence, min_above, min_below, look_back, look_ahead, max_size};
    return amp_gate_impl(ctx, x, count, n, ld, a, hipass, out, smoothed);
  });
}

int fluhip_bufampgate_f32(fluhip_ctx* ctx, const float* audio, int64_t count, int64_t channels, int64_t n, int64_t start_frame,
                          int64_t ramp_up, int64_t ramp_down, double on, double off, int64_t min_slice, int64_t min_silence,
                          int64_t min_above, int64_t min_below, int64_t look_back, int64_t look_ahead, double high_pass_freq,
                          double sample_rate, int64_t max_size, int64_t* indices, int64_t capacity, int64_t* counts)
{
  return guarded(ctx, [&] {
    const GateParams a{ramp_up, ramp_down, on, off, min_slice, min_silence, min_above, min_below, look_back, look_ahead, max_size};
    return bufampgate_impl(ctx, audio, count, channels, n, start_frame, a, high_pass_freq, sample_rate, indices, capacity, counts);
  });
}

} // extern "C"
