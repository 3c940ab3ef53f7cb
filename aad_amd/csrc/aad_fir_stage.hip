/* aad_fir_stage.hip - host side of the FIR stages behind a window decode (include/aad_hip.h "resample", "reverberation") and of
 * the spectrogram stage behind any of them ("spectrogram"): every AADHip_Resampler*, AADHip_Convolver* and AADHip_Spectrogram*
 * entry point.  No kernel is instantiated here: the launches are aad_resample.hip's, aad_resample_wide.hip's, aad_convolve.hip's,
 * aad_convolve_stats.hip's, aad_spectrogram.hip's and aad_spectrogram_mix.hip's.  A stage is made by its own Create; what a Resolve or
 * a Run refuses is one rule for both (aad_fir_stage.h), asked through the few members a stage states about itself, and every
 * launch ends in `launched`. */
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>
#include <algorithm>
#include <new>
#include <vector>

#include "aad_convolve.hip.h"
#include "aad_fir_stage.h"
#include "aad_hip_context.hip.h"
#include "aad_resample.hip.h"
#include "aad_spectrogram.hip.h"

static_assert(sizeof(AADHipResampleLane) == sizeof(aad::ResampleLane), "lane record layout");
static_assert(sizeof(AADHipConvolveLane) == sizeof(aad::ConvolveLane), "lane record layout");

/* What the shared checks ask of a stage: ctx; kName and kFrames, the stage and why it refuses a frame count, for last_error;
 * kTile, the output frames of a workgroup; source_frames, false where `frames` is refused; lds_bytes, what a launch that can
 * be refused asked for; fill, the stage's own fields of its kernels' arguments.
 * AADHip_ResamplerCreate: the banks on the host (AADHip_ResamplerBank reads them) and on the device, the select table */
struct AADHipResampler {
  static constexpr const char *kName = "resampler", *kFrames = "0, or (T - 1) M >= 2^31 for a bank";
  static constexpr uint32_t kTile = aad::kResampleTile;
  AADHipContext *ctx = nullptr;
  uint32_t num_streams = 0, variants = 0;
  std::vector<aad::ResampleBankDesc> banks; /* one per ratio, in the caller's order */
  std::vector<int16_t> coefficients; /* bank r's L * K taps at banks[r].offset: what AADHip_ResamplerBank returns */
  uint64_t bank_elements = 0, span_elements = 0; /* the FIR kernel's LDS, in int16 elements: the largest bank and span */
  /* AADHip_ResamplerCreateWide: the runs launch aad_resample_wide.hip's kernels; round: R of their gather path
   * (resample_gather_round of the gathered bank with the most taps), 0 when every bank is resident */
  bool wide = false;
  uint32_t round = 0;
  uint16_t *d_select = nullptr, *d_lead = nullptr;
  aad::ResampleBankDesc *d_banks = nullptr;
  int16_t *d_coefficients = nullptr;

  /* T_src = max over the banks of ((T - 1) M) div L + K; false for T == 0 and a bank with (T - 1) M >= 2^31 */
  bool source_frames(uint32_t frames, uint32_t *source_frames) const
  {
    uint64_t most = 0, n = 0;
    for (const aad::ResampleBankDesc &b : banks) {
      if (!aad::resample_source_frames(frames, b.L, b.M, b.K, &n)) return false;
      most = std::max(most, n);
    }
    *source_frames = (uint32_t)most; /* < 2^31 + 256 */
    return true;
  }
  /* bytes of LDS a FIR launch asks for, the statistics scratch aside: bank (or a round's rows), span, phase index */
  uint32_t lds_bytes() const { return (uint32_t)(2 * (bank_elements + span_elements) + 4 * round); }
  void fill(aad::ResampleMixArgs *m) const
  {
    m->r.banks = d_banks;
    m->r.coefficients = d_coefficients;
    m->r.num_banks = (uint32_t)banks.size();
    m->r.bank_elements = (uint32_t)bank_elements;
    m->r.span_elements = (uint32_t)span_elements;
    m->round = round;
  }
};

/* AADHip_ConvolverCreate: the responses on the host (AADHip_ConvolverResponse reads them) and, as byte planes, on the device */
struct AADHipConvolver {
  static constexpr const char *kName = "convolver", *kFrames = "0, or T + K - 1 past 32 bits";
  static constexpr uint32_t kTile = aad::kConvolveTile;
  AADHipContext *ctx = nullptr;
  std::vector<aad::convolve::ResponseDesc> responses; /* offset: the first tap in `taps` */
  std::vector<int16_t> taps;
  uint32_t max_taps = 0; /* the longest response: T_src = T + max_taps - 1 */
  uint32_t *d_lead = nullptr;
  aad::convolve::ResponseDesc *d_responses = nullptr; /* offset: the first byte in d_planes */
  int8_t *d_planes = nullptr;

  bool source_frames(uint32_t frames, uint32_t *source_frames) const
  {
    uint64_t n = 0;
    if (!aad::convolve_source_frames(frames, max_taps, &n) || n > UINT32_MAX) return false;
    *source_frames = (uint32_t)n;
    return true;
  }
  uint32_t lds_bytes() const { return 0; } /* static LDS alone: no launch of the stage is refused */
  template <class Args> /* GainArgs, StatsArgs */
  void fill(Args *m) const
  {
    m->r.responses = d_responses;
    m->r.planes = d_planes;
    m->r.num_responses = (uint32_t)responses.size();
  }
};

namespace {

uint64_t address(const void *p) { return (uint64_t)reinterpret_cast<uintptr_t>(p); }

/* The tail of every launch: ok false - the launch function refused the stage's LDS - or what the launch left behind.  `run`
 * names the call in last_error, here and below: "resolve", "run", "run with gain", "run with statistics". */
template <class Stage>
AADApiResult launched(Stage *s, const char *run, bool ok)
{
  const hipError_t e = ok ? hipGetLastError() : hipSuccess;
  if (ok && e == hipSuccess) return AAD_APIRESULT_OK; /* nothing is formatted on the way of a good call */
  char *error = s->ctx->last_error;
  if (ok) snprintf(error, sizeof(s->ctx->last_error), "%s %s launch: %s", Stage::kName, run, hipGetErrorString(e));
  else snprintf(error, sizeof(s->ctx->last_error), "%s %s: the device refuses %llu bytes of LDS for a workgroup", Stage::kName, run,
                (unsigned long long)s->lds_bytes());
  return AAD_APIRESULT_NG;
}

/* A Resolve of either stage: what it refuses, then - with the context's device selected, and unless the run is empty - `launch`,
 * which ends in `launched` */
template <class Stage, class Launch>
AADApiResult resolve(Stage *s, uint64_t num_windows, const void *windows, const void *selector, uint32_t frames,
                     const void *source_windows, const void *lanes, Launch launch)
{
  uint32_t source_frames = 0;
  if (!s->source_frames(frames, &source_frames) ||
      !aad::fir_resolve_ok(num_windows, address(windows), address(selector), address(source_windows), address(lanes))) {
    snprintf(s->ctx->last_error, sizeof(s->ctx->last_error), "%s resolve: a null or unaligned table, %u frames (%s), or %llu windows",
             Stage::kName, frames, Stage::kFrames, (unsigned long long)num_windows);
    return AAD_APIRESULT_INVALID_ARGUMENT;
  }
  DeviceGuard guard(s->ctx);
  if (!guard.ok) return AAD_APIRESULT_NG;
  return num_windows == 0 ? AAD_APIRESULT_OK : launch();
}

/* Every FIR run of either stage: what AADHip_ResamplerRun refuses (out_optional: AADHip_ResamplerRunStats), the kernel's
 * arguments - the rows' into m->r and the stage's own, which `launch` reads - then `launch` */
template <class Stage, class Lane, class Args, class Launch>
AADApiResult run_rows(Stage *s, const char *run, uint64_t num_windows, uint32_t channels, const int16_t *device_source_rows,
                      uint32_t source_frames, const Lane *device_lanes, uint32_t frames, int32_t sample_type, void *device_out,
                      bool out_optional, Args *m, Launch launch)
{
  uint32_t needed = 0;
  aad::FirRows f = {false, 0, 0};
  if (window_sample_type_ok(sample_type) && channels != 0 && s->source_frames(frames, &needed))
    f = aad::fir_rows(num_windows, channels, frames, source_frames, needed, sample_type == AAD_HIP_SAMPLE_FLOAT32 ? 4 : 2,
                      address(device_source_rows), address(device_lanes), address(device_out), out_optional, Stage::kTile);
  if (!f.ok) {
    snprintf(s->ctx->last_error, sizeof(s->ctx->last_error),
             "%s %s: an unknown sample type, a null or unaligned pointer, 0 channels, %u frames (%s), source rows of %u frames where "
             "%u are needed, or %llu windows x %u channels x frames past 64 bits",
             Stage::kName, run, frames, Stage::kFrames, source_frames, needed, (unsigned long long)num_windows, channels);
    return AAD_APIRESULT_INVALID_ARGUMENT;
  }
  m->r.src = device_source_rows;
  m->r.lanes = reinterpret_cast<decltype(m->r.lanes)>(device_lanes);
  m->r.out = device_out;
  m->r.rows = f.rows;
  m->r.channels = channels;
  m->r.frames = frames;
  m->r.source_frames = source_frames;
  m->r.tiles = f.tiles;
  s->fill(m);
  DeviceGuard guard(s->ctx);
  if (!guard.ok) return AAD_APIRESULT_NG;
  return num_windows == 0 ? AAD_APIRESULT_OK : launch();
}

/* A run with gain of either stage: what it refuses in front of run_rows, the tables into `m`, and launch(add) */
template <class Stage, class Lane, class Args, class Launch>
AADApiResult run_gain(Stage *s, uint64_t num_windows, uint32_t channels, const int16_t *device_source_rows, uint32_t source_frames,
                      const Lane *device_lanes, const struct AADHipWindowSpan *device_spans, uint32_t frames, int32_t sample_type,
                      void *device_out, const float *device_gain, int32_t mode, Args *m, Launch launch)
{
  if (!aad::fir_gain_ok(sample_type, mode, address(device_gain), address(device_spans))) {
    snprintf(s->ctx->last_error, sizeof(s->ctx->last_error),
             "%s run with gain: int16 rows, a mode that is neither STORE nor ADD, a gain table off 4-byte or a span table off 8-byte "
             "alignment", Stage::kName);
    return AAD_APIRESULT_INVALID_ARGUMENT;
  }
  m->spans = reinterpret_cast<const uint64_t *>(device_spans);
  m->gain = device_gain;
  const bool add = mode == AAD_HIP_WINDOW_GAIN_ADD;
  return run_rows(s, "run with gain", num_windows, channels, device_source_rows, source_frames, device_lanes, frames, sample_type,
                  device_out, false, m, [&] { return launch(add); });
}

/* A run with statistics of either stage: what it refuses in front of run_rows, the tables into `m`, the clear of the records on
 * the context's stream, and launch() */
template <class Stage, class Lane, class Args, class Launch>
AADApiResult run_stats(Stage *s, uint64_t num_windows, uint32_t channels, const int16_t *device_source_rows, uint32_t source_frames,
                       const Lane *device_lanes, const struct AADHipRowStats *device_source_stats,
                       const struct AADHipWindowSpan *device_spans, uint32_t frames, int32_t sample_type, void *device_out,
                       struct AADHipRowStats *device_stats, Args *m, Launch launch)
{
  const aad::WindowStatsTable t = aad::window_stats_table(num_windows, channels, address(device_stats));
  const aad::WindowStatsTable ts = aad::window_stats_table(num_windows, channels, address(device_source_stats));
  if (!t.ok || !ts.ok || (address(device_spans) & 7u) != 0 || (device_out != nullptr && device_spans != nullptr)) {
    snprintf(s->ctx->last_error, sizeof(s->ctx->last_error),
             "%s run with statistics: a null or unaligned statistics table, a span table off 8-byte alignment, rows together "
             "with spans, or %llu windows x %u channels x 32 bytes overflow 64 bits",
             Stage::kName, (unsigned long long)num_windows, channels);
    return AAD_APIRESULT_INVALID_ARGUMENT;
  }
  m->spans = reinterpret_cast<const uint64_t *>(device_spans);
  m->source_stats = reinterpret_cast<const unsigned long long *>(device_source_stats);
  m->stats = reinterpret_cast<unsigned long long *>(device_stats);
  return run_rows(s, "run with statistics", num_windows, channels, device_source_rows, source_frames, device_lanes, frames, sample_type,
                  device_out, true, m, [&] {
                    if (!hip_ok(s->ctx, hipMemsetAsync(device_stats, 0, t.bytes, s->ctx->stream), "hipMemsetAsync")) return AAD_APIRESULT_NG;
                    return launch();
                  });
}

/* a Destroy: the stage's device memory, once the context's stream has drained, and the stage */
template <class Stage>
void destroy(Stage *s, std::initializer_list<void *> device)
{
  DeviceGuard guard(s->ctx);
  if (guard.ok) {
    (void)hipStreamSynchronize(s->ctx->stream);
    for (void *p : device) (void)hipFree(p); /* a null pointer: no operation */
  }
  delete s;
}

/* AADHip_ResamplerCreate, and with `wide` AADHip_ResamplerCreateWide: the same resampler but for the limits of a ratio and the
 * kernels its runs launch */
AADApiResult resampler_create(struct AADHipContext *ctx, uint32_t num_ratios, const struct AADHipResampleRatio *ratios, uint32_t num_streams,
                              uint32_t variants, const uint16_t *select, struct AADHipResampler **resampler, bool wide)
{
  if (ctx == nullptr || resampler == nullptr || ratios == nullptr || num_ratios == 0 || num_ratios >= aad::kResampleNoBank ||
      variants == 0 || (num_streams != 0 && select == nullptr))
    return AAD_APIRESULT_INVALID_ARGUMENT;
  *resampler = nullptr;
  const uint64_t entries = (uint64_t)num_streams * variants;
  for (uint64_t i = 0; i < entries; i++)
    if (select[i] != aad::kResampleNoBank && select[i] >= num_ratios) return AAD_APIRESULT_INVALID_ARGUMENT;
  AADHipResampler *r = new (std::nothrow) AADHipResampler();
  if (r == nullptr) return AAD_APIRESULT_NG;
  r->ctx = ctx;
  r->num_streams = num_streams;
  r->variants = variants;
  r->wide = wide;
  std::vector<uint16_t> lead(num_ratios);
  uint64_t gathered_stride = 0; /* the longest row of a gathered bank, in int16 elements */
  /* the device's copy: a resident bank as on the host, a gathered one with its rows resample_gather_pitch(K) apart on 16-byte
   * boundaries; device_banks[r].offset is into it */
  std::vector<int16_t> image;
  std::vector<aad::ResampleBankDesc> device_banks;
  for (uint32_t i = 0; i < num_ratios; i++) {
    aad::ResampleRatio q;
    if (!aad::resample_reduce(ratios[i].up, ratios[i].down, &q) ||
        !(wide ? aad::resample_wide_shape_ok(q.L, q.M) : aad::resample_shape_ok(q.L, q.M))) {
      snprintf(ctx->last_error, sizeof(ctx->last_error),
               wide ? "wide resampler: ratio %u (%u / %u) is zero, or has more than 32768 phases, 256 taps or 2 MiB of bank"
                    : "resampler: ratio %u (%u / %u) is zero, or has more than 1024 phases, 256 taps or 65536 bytes of bank",
               i, ratios[i].up, ratios[i].down);
      delete r;
      return AAD_APIRESULT_INVALID_ARGUMENT;
    }
    const uint32_t K = (uint32_t)aad::resample_taps(q.L, q.M);
    const size_t at = r->coefficients.size();
    const bool resident = aad::resample_bank_resident(q.L, K);
    const uint32_t pitch = resident ? K : aad::resample_gather_pitch(K);
    const size_t image_at = resident ? image.size() : (image.size() + 7) & ~(size_t)7;
    if (image_at + (uint64_t)q.L * pitch >= aad::kResampleMaxCoefficients) { /* a wide resampler alone can get here */
      snprintf(ctx->last_error, sizeof(ctx->last_error), "wide resampler: the banks up to ratio %u hold 2^31 coefficients or more", i);
      delete r;
      return AAD_APIRESULT_INVALID_ARGUMENT;
    }
    r->coefficients.resize(at + (size_t)q.L * K);
    if (!aad::resample_build_bank(q.L, q.M, r->coefficients.data() + at)) {
      snprintf(ctx->last_error, sizeof(ctx->last_error), "resampler: ratio %u (%u / %u) has a phase with sum |h| above 65535", i,
               ratios[i].up, ratios[i].down);
      delete r;
      return AAD_APIRESULT_INVALID_ARGUMENT;
    }
    r->banks.push_back(aad::ResampleBankDesc{q.L, q.M, K, (uint32_t)at});
    device_banks.push_back(aad::ResampleBankDesc{q.L, q.M, K, (uint32_t)image_at});
    image.resize(image_at + (size_t)q.L * pitch, 0);
    for (uint32_t p = 0; p < q.L; p++)
      memcpy(image.data() + image_at + (size_t)p * pitch, r->coefficients.data() + at + (size_t)p * K, sizeof(int16_t) * K);
    lead[i] = (uint16_t)(K / 2 - 1);
    if (resident) {
      r->bank_elements = std::max<uint64_t>(r->bank_elements, (uint64_t)q.L * aad::resample_lds_stride(K));
    } else { /* gathered: the round of the bank with the most taps is the smallest */
      const uint32_t round = aad::resample_gather_round(K);
      r->round = r->round == 0 ? round : std::min(r->round, round);
      gathered_stride = std::max<uint64_t>(gathered_stride, aad::resample_lds_stride(K));
    }
    r->span_elements = std::max<uint64_t>(r->span_elements, aad::resample_span_elements(q.L, q.M, K));
  }
  r->bank_elements = std::max<uint64_t>(r->bank_elements, r->round * gathered_stride);
  DeviceGuard guard(ctx);
  if (!guard.ok || !upload(ctx, &r->d_select, select, (size_t)entries) || !upload(ctx, &r->d_lead, lead.data(), lead.size()) ||
      !upload(ctx, &r->d_banks, device_banks.data(), device_banks.size()) ||
      !upload(ctx, &r->d_coefficients, image.data(), image.size())) {
    AADHip_ResamplerDestroy(r);
    return AAD_APIRESULT_NG;
  }
  *resampler = r;
  return AAD_APIRESULT_OK;
}
} /* namespace */

AADApiResult AADHip_ResamplerCreate(struct AADHipContext *ctx, uint32_t num_ratios, const struct AADHipResampleRatio *ratios,
                                    uint32_t num_streams, uint32_t variants, const uint16_t *select, struct AADHipResampler **resampler)
{
  return resampler_create(ctx, num_ratios, ratios, num_streams, variants, select, resampler, false);
}

AADApiResult AADHip_ResamplerCreateWide(struct AADHipContext *ctx, uint32_t num_ratios, const struct AADHipResampleRatio *ratios,
                                        uint32_t num_streams, uint32_t variants, const uint16_t *select, struct AADHipResampler **resampler)
{
  return resampler_create(ctx, num_ratios, ratios, num_streams, variants, select, resampler, true);
}

void AADHip_ResamplerDestroy(struct AADHipResampler *r)
{
  if (r != nullptr) destroy(r, {r->d_select, r->d_lead, r->d_banks, r->d_coefficients});
}

AADApiResult AADHip_ResamplerBank(const struct AADHipResampler *r, uint32_t ratio, uint32_t *L, uint32_t *M, uint32_t *taps,
                                  int16_t *coefficients, uint64_t capacity)
{
  if (r == nullptr || ratio >= r->banks.size() || L == nullptr || M == nullptr || taps == nullptr) return AAD_APIRESULT_INVALID_ARGUMENT;
  const aad::ResampleBankDesc &b = r->banks[ratio];
  if (coefficients != nullptr && capacity < (uint64_t)b.L * b.K) return AAD_APIRESULT_INSUFFICIENT_BUFFER;
  *L = b.L;
  *M = b.M;
  *taps = b.K;
  if (coefficients != nullptr) memcpy(coefficients, r->coefficients.data() + b.offset, sizeof(int16_t) * b.L * b.K);
  return AAD_APIRESULT_OK;
}

AADApiResult AADHip_ResamplerSourceFrames(const struct AADHipResampler *r, uint32_t frames, uint32_t *source_frames)
{
  if (r == nullptr || source_frames == nullptr || !r->source_frames(frames, source_frames)) return AAD_APIRESULT_INVALID_ARGUMENT;
  return AAD_APIRESULT_OK;
}

AADApiResult AADHip_ResamplerResolve(struct AADHipResampler *r, uint64_t num_windows, const struct AADHipWindow *device_windows,
                                     const int64_t *device_variant, uint32_t frames, struct AADHipWindow *device_source_windows,
                                     struct AADHipResampleLane *device_lanes)
{
  if (r == nullptr) return AAD_APIRESULT_INVALID_ARGUMENT;
  return resolve(r, num_windows, device_windows, device_variant, frames, device_source_windows, device_lanes, [&] {
    aad::ResampleResolveArgs a;
    a.windows = reinterpret_cast<const uint64_t *>(device_windows);
    a.variant = reinterpret_cast<const uint64_t *>(device_variant);
    a.select = r->d_select;
    a.lead = r->d_lead;
    a.num_windows = num_windows;
    a.num_streams = r->num_streams;
    a.variants = r->variants;
    a.source_windows = reinterpret_cast<uint64_t *>(device_source_windows);
    a.lanes = reinterpret_cast<aad::ResampleLane *>(device_lanes);
    aad::launch_resample_resolve(a, r->ctx->stream);
    return launched(r, "resolve", true);
  });
}

AADApiResult AADHip_ResamplerRun(struct AADHipResampler *r, uint64_t num_windows, uint32_t channels, const int16_t *device_source_rows,
                                 uint32_t source_frames, const struct AADHipResampleLane *device_lanes, uint32_t frames,
                                 int32_t sample_type, void *device_out)
{
  if (r == nullptr) return AAD_APIRESULT_INVALID_ARGUMENT;
  aad::ResampleMixArgs m = {}; /* a wide resampler's kernels take the plain run's arguments in it */
  const auto launch = [&] {
    return launched(r, "run", r->wide ? aad::launch_resample_rows_wide(m, sample_type, r->lds_bytes(), r->ctx->stream)
                                      : aad::launch_resample_rows(m.r, sample_type, r->lds_bytes(), r->ctx->stream));
  };
  return run_rows(r, "run", num_windows, channels, device_source_rows, source_frames, device_lanes, frames, sample_type, device_out,
                  false, &m, launch);
}

AADApiResult AADHip_ResamplerRunGain(struct AADHipResampler *r, uint64_t num_windows, uint32_t channels,
                                     const int16_t *device_source_rows, uint32_t source_frames,
                                     const struct AADHipResampleLane *device_lanes, const struct AADHipWindowSpan *device_spans,
                                     uint32_t frames, int32_t sample_type, void *device_out, const float *device_gain, int32_t mode)
{
  if (r == nullptr) return AAD_APIRESULT_INVALID_ARGUMENT;
  aad::ResampleMixArgs m = {};
  const auto rows = r->wide ? aad::launch_resample_rows_gain_wide : aad::launch_resample_rows_gain;
  const auto launch = [&](bool add) { return launched(r, "run with gain", rows(m, sample_type, add, r->lds_bytes(), r->ctx->stream)); };
  return run_gain(r, num_windows, channels, device_source_rows, source_frames, device_lanes, device_spans, frames, sample_type,
                  device_out, device_gain, mode, &m, launch);
}

AADApiResult AADHip_ResamplerRunStats(struct AADHipResampler *r, uint64_t num_windows, uint32_t channels,
                                      const int16_t *device_source_rows, uint32_t source_frames,
                                      const struct AADHipResampleLane *device_lanes, const struct AADHipRowStats *device_source_stats,
                                      const struct AADHipWindowSpan *device_spans, uint32_t frames, int32_t sample_type,
                                      void *device_out, struct AADHipRowStats *device_stats)
{
  if (r == nullptr) return AAD_APIRESULT_INVALID_ARGUMENT;
  aad::ResampleMixArgs m = {};
  const auto rows = r->wide ? aad::launch_resample_rows_stats_wide : aad::launch_resample_rows_stats;
  const auto launch = [&] { return launched(r, "run with statistics", rows(m, sample_type, r->lds_bytes(), r->ctx->stream)); };
  return run_stats(r, num_windows, channels, device_source_rows, source_frames, device_lanes, device_source_stats, device_spans, frames,
                   sample_type, device_out, device_stats, &m, launch);
}

AADApiResult AADHip_ConvolverCreate(struct AADHipContext *ctx, uint32_t num_responses, const float *const *taps, const uint32_t *lengths,
                                    const int32_t *delays, struct AADHipConvolver **convolver)
{
  if (ctx == nullptr || convolver == nullptr || taps == nullptr || lengths == nullptr || num_responses == 0)
    return AAD_APIRESULT_INVALID_ARGUMENT;
  *convolver = nullptr;
  AADHipConvolver *c = new (std::nothrow) AADHipConvolver();
  if (c == nullptr) return AAD_APIRESULT_NG;
  c->ctx = ctx;
  std::vector<uint32_t> lead(num_responses);
  std::vector<int8_t> planes;
  std::vector<aad::convolve::ResponseDesc> device_responses;
  for (uint32_t i = 0; i < num_responses; i++) {
    const uint32_t K = lengths[i];
    const size_t at = c->taps.size();
    c->taps.resize(at + (K <= aad::kConvolveMaxTaps ? K : 0));
    uint32_t q = 0, delay = 0;
    if (taps[i] == nullptr || !aad::convolve_quantise(taps[i], K, delays != nullptr ? delays[i] : -1, c->taps.data() + at, &q, &delay)) {
      snprintf(ctx->last_error, sizeof(ctx->last_error),
               "convolver: response %u has %u taps (1 ... 32768), a tap that is not finite or past 32639 in magnitude, or a delay "
               "outside its taps", i, K);
      delete c;
      return AAD_APIRESULT_INVALID_ARGUMENT;
    }
    const uint32_t steps = aad::convolve_steps(K);
    const size_t image_at = planes.size();
    planes.resize(image_at + (size_t)steps * aad::kConvolveStepBytes);
    aad::convolve_build_planes(c->taps.data() + at, K, planes.data() + image_at);
    const int64_t bias = aad::convolve_bias(c->taps.data() + at, K);
    c->responses.push_back(aad::convolve::ResponseDesc{K, q, delay, steps, (uint64_t)at, bias});
    device_responses.push_back(aad::convolve::ResponseDesc{K, q, delay, steps, (uint64_t)image_at, bias});
    lead[i] = K - 1 - delay;
    c->max_taps = std::max(c->max_taps, K);
  }
  DeviceGuard guard(ctx);
  if (!guard.ok || !upload(ctx, &c->d_lead, lead.data(), lead.size()) ||
      !upload(ctx, &c->d_responses, device_responses.data(), device_responses.size()) ||
      !upload(ctx, &c->d_planes, planes.data(), planes.size())) {
    AADHip_ConvolverDestroy(c);
    return AAD_APIRESULT_NG;
  }
  *convolver = c;
  return AAD_APIRESULT_OK;
}

void AADHip_ConvolverDestroy(struct AADHipConvolver *c)
{
  if (c != nullptr) destroy(c, {c->d_lead, c->d_responses, c->d_planes});
}

AADApiResult AADHip_ConvolverResponse(const struct AADHipConvolver *c, uint32_t response, uint32_t *num_taps, uint32_t *scale,
                                      uint32_t *delay, int16_t *taps, uint64_t capacity)
{
  if (c == nullptr || response >= c->responses.size() || num_taps == nullptr || scale == nullptr || delay == nullptr)
    return AAD_APIRESULT_INVALID_ARGUMENT;
  const aad::convolve::ResponseDesc &d = c->responses[response];
  if (taps != nullptr && capacity < d.K) return AAD_APIRESULT_INSUFFICIENT_BUFFER;
  *num_taps = d.K;
  *scale = d.q;
  *delay = d.delay;
  if (taps != nullptr) memcpy(taps, c->taps.data() + d.offset, sizeof(int16_t) * d.K);
  return AAD_APIRESULT_OK;
}

AADApiResult AADHip_ConvolverSourceFrames(const struct AADHipConvolver *c, uint32_t frames, uint32_t *source_frames)
{
  if (c == nullptr || source_frames == nullptr || !c->source_frames(frames, source_frames)) return AAD_APIRESULT_INVALID_ARGUMENT;
  return AAD_APIRESULT_OK;
}

AADApiResult AADHip_ConvolverResolve(struct AADHipConvolver *c, uint64_t num_windows, const struct AADHipWindow *device_windows,
                                     const int64_t *device_response, uint32_t frames, struct AADHipWindow *device_source_windows,
                                     struct AADHipConvolveLane *device_lanes)
{
  if (c == nullptr) return AAD_APIRESULT_INVALID_ARGUMENT;
  return resolve(c, num_windows, device_windows, device_response, frames, device_source_windows, device_lanes, [&] {
    aad::convolve::ResolveArgs a;
    a.windows = reinterpret_cast<const uint64_t *>(device_windows);
    a.response = reinterpret_cast<const uint64_t *>(device_response);
    a.lead = c->d_lead;
    a.num_windows = num_windows;
    a.num_responses = (uint32_t)c->responses.size();
    a.source_windows = reinterpret_cast<uint64_t *>(device_source_windows);
    a.lanes = reinterpret_cast<aad::ConvolveLane *>(device_lanes);
    aad::convolve::launch_resolve(a, c->ctx->stream);
    return launched(c, "resolve", true);
  });
}

AADApiResult AADHip_ConvolverRun(struct AADHipConvolver *c, uint64_t num_windows, uint32_t channels, const int16_t *device_source_rows,
                                 uint32_t source_frames, const struct AADHipConvolveLane *device_lanes, uint32_t frames,
                                 int32_t sample_type, void *device_out)
{
  if (c == nullptr) return AAD_APIRESULT_INVALID_ARGUMENT;
  aad::convolve::GainArgs m = {}; /* m.r: the run's arguments */
  const auto launch = [&] { aad::convolve::launch_rows(m.r, sample_type, c->ctx->stream); return launched(c, "run", true); };
  return run_rows(c, "run", num_windows, channels, device_source_rows, source_frames, device_lanes, frames, sample_type, device_out,
                  false, &m, launch);
}

AADApiResult AADHip_ConvolverRunGain(struct AADHipConvolver *c, uint64_t num_windows, uint32_t channels,
                                     const int16_t *device_source_rows, uint32_t source_frames,
                                     const struct AADHipConvolveLane *device_lanes, const struct AADHipWindowSpan *device_spans,
                                     uint32_t frames, int32_t sample_type, void *device_out, const float *device_gain, int32_t mode)
{
  if (c == nullptr) return AAD_APIRESULT_INVALID_ARGUMENT;
  aad::convolve::GainArgs m = {};
  const auto launch = [&](bool add) {
    aad::convolve::launch_rows_gain(m, sample_type, add, c->ctx->stream);
    return launched(c, "run with gain", true);
  };
  return run_gain(c, num_windows, channels, device_source_rows, source_frames, device_lanes, device_spans, frames, sample_type,
                  device_out, device_gain, mode, &m, launch);
}

AADApiResult AADHip_ConvolverRunStats(struct AADHipConvolver *c, uint64_t num_windows, uint32_t channels,
                                      const int16_t *device_source_rows, uint32_t source_frames,
                                      const struct AADHipConvolveLane *device_lanes, const struct AADHipRowStats *device_source_stats,
                                      const struct AADHipWindowSpan *device_spans, uint32_t frames, int32_t sample_type,
                                      void *device_out, struct AADHipRowStats *device_stats)
{
  if (c == nullptr) return AAD_APIRESULT_INVALID_ARGUMENT;
  aad::convolve::StatsArgs m = {};
  const auto launch = [&] {
    aad::convolve_levels::launch_rows_stats(m, sample_type, c->ctx->stream);
    return launched(c, "run with statistics", true);
  };
  return run_stats(c, num_windows, channels, device_source_rows, source_frames, device_lanes, device_source_stats, device_spans, frames,
                   sample_type, device_out, device_stats, &m, launch);
}

/* ---- spectrogram (include/aad_hip.h "spectrogram") ------------------------------------------------------------------------------ */

/* AADHip_SpectrogramCreate: the quantised matrices on the host (AADHip_SpectrogramCoefficients reads them) and, as byte planes
 * with their column constants and the filters' bands, packed weights and per-pair lists, on the device */
struct AADHipSpectrogram {
  static constexpr const char *kName = "spectrogram";
  AADHipContext *ctx = nullptr;
  uint32_t n_fft = 0, win = 0, hop = 0, q = 0, num_filters = 0;
  aad::SpectrumGeometry g = {};
  std::vector<int16_t> cos_sin; /* [W][B][2] */
  int8_t *d_planes = nullptr;
  long long *d_consts = nullptr;
  aad::SpectrumBand *d_bands = nullptr;
  float *d_weights = nullptr;
  uint32_t *d_tile_first = nullptr, *d_tile_list = nullptr;
  uint32_t lds_bytes() const { return aad::spectrum_lds_bytes(g, num_filters != 0); }
};

AADApiResult AADHip_SpectrogramCreate(struct AADHipContext *ctx, uint32_t n_fft, uint32_t win_length, uint32_t hop, const float *window,
                                      uint32_t num_filters, const float *filters, struct AADHipSpectrogram **spectrogram)
{
  if (ctx == nullptr || spectrogram == nullptr) return AAD_APIRESULT_INVALID_ARGUMENT;
  *spectrogram = nullptr;
  if (window == nullptr || !aad::spectrum_shape_ok(n_fft, win_length, hop) || (filters == nullptr) != (num_filters == 0)) {
    snprintf(ctx->last_error, sizeof(ctx->last_error),
             "spectrogram: n_fft %u, window %u, hop %u (1 <= window <= n_fft <= 4096, hop >= 1), a null window, or filters without a "
             "count", n_fft, win_length, hop);
    return AAD_APIRESULT_INVALID_ARGUMENT;
  }
  AADHipSpectrogram *s = new (std::nothrow) AADHipSpectrogram();
  if (s == nullptr) return AAD_APIRESULT_NG;
  s->ctx = ctx;
  s->n_fft = n_fft;
  s->win = win_length;
  s->hop = hop;
  s->num_filters = num_filters;
  s->g = aad::spectrum_geometry(win_length, hop);
  const uint32_t B = aad::spectrum_bins(n_fft), pairs = aad::spectrum_pairs(n_fft);
  s->cos_sin.resize((size_t)win_length * B * 2);
  std::vector<aad::SpectrumBand> bands(num_filters);
  uint64_t total = 0;
  if (!aad::spectrum_quantise(window, n_fft, win_length, s->cos_sin.data(), &s->q) ||
      !aad::spectrum_bands(filters, num_filters, B, bands.data(), &total)) {
    snprintf(ctx->last_error, sizeof(ctx->last_error),
             "spectrogram: a window value that is not finite or a coefficient past 32639 at scale 0, or a filter weight that is not "
             "finite or nonzero below 2^-60");
    delete s;
    return AAD_APIRESULT_INVALID_ARGUMENT;
  }
  std::vector<int8_t> planes((size_t)aad::spectrum_plane_bytes(n_fft, win_length));
  aad::spectrum_build_planes(s->cos_sin.data(), n_fft, win_length, planes.data());
  std::vector<long long> consts((size_t)32 * pairs);
  static_assert(sizeof(long long) == sizeof(int64_t), "the column constants");
  aad::spectrum_column_constants(s->cos_sin.data(), n_fft, win_length, reinterpret_cast<int64_t *>(consts.data()));
  std::vector<float> weights((size_t)total);
  aad::spectrum_pack_weights(filters, num_filters, B, bands.data(), weights.data());
  std::vector<uint32_t> first(pairs + 1);
  aad::spectrum_tile_lists(bands.data(), num_filters, B, pairs, first.data(), nullptr);
  std::vector<uint32_t> list(first[pairs]);
  aad::spectrum_tile_lists(bands.data(), num_filters, B, pairs, first.data(), list.data());
  DeviceGuard guard(ctx);
  if (!guard.ok || !upload(ctx, &s->d_planes, planes.data(), planes.size()) || !upload(ctx, &s->d_consts, consts.data(), consts.size()) ||
      !upload(ctx, &s->d_bands, bands.data(), bands.size()) || !upload(ctx, &s->d_weights, weights.data(), weights.size()) ||
      !upload(ctx, &s->d_tile_first, first.data(), first.size()) || !upload(ctx, &s->d_tile_list, list.data(), list.size())) {
    AADHip_SpectrogramDestroy(s);
    return AAD_APIRESULT_NG;
  }
  *spectrogram = s;
  return AAD_APIRESULT_OK;
}

void AADHip_SpectrogramDestroy(struct AADHipSpectrogram *s)
{
  if (s != nullptr) destroy(s, {s->d_planes, s->d_consts, s->d_bands, s->d_weights, s->d_tile_first, s->d_tile_list});
}

AADApiResult AADHip_SpectrogramFrames(const struct AADHipSpectrogram *s, uint32_t frames, uint32_t *num_frames)
{
  if (s == nullptr || num_frames == nullptr || !aad::spectrum_frames(frames, s->win, s->hop, num_frames)) return AAD_APIRESULT_INVALID_ARGUMENT;
  return AAD_APIRESULT_OK;
}

AADApiResult AADHip_SpectrogramCoefficients(const struct AADHipSpectrogram *s, uint32_t *scale, int16_t *cos_sin, uint64_t capacity)
{
  if (s == nullptr || scale == nullptr) return AAD_APIRESULT_INVALID_ARGUMENT;
  if (cos_sin != nullptr && capacity < s->cos_sin.size()) return AAD_APIRESULT_INSUFFICIENT_BUFFER;
  *scale = s->q;
  if (cos_sin != nullptr) memcpy(cos_sin, s->cos_sin.data(), sizeof(int16_t) * s->cos_sin.size());
  return AAD_APIRESULT_OK;
}

namespace {

/* the kernels' arguments of a run the stage's rule has passed: the handle's and the run's */
aad::spectrum::Args spectrogram_args(const AADHipSpectrogram *s, const aad::SpectrumRows &r, uint64_t num_rows, const int16_t *device_rows,
                                     uint64_t row_pitch, uint32_t frames, float *device_out)
{
  aad::spectrum::Args a = {};
  a.rows = device_rows;
  a.row_pitch = row_pitch;
  a.num_rows = num_rows;
  a.frames = frames;
  a.num_frames = r.num_frames;
  a.hop = s->hop;
  a.steps = aad::spectrum_steps(s->win);
  a.pairs = aad::spectrum_pairs(s->n_fft);
  a.bins = aad::spectrum_bins(s->n_fft);
  a.q = s->q;
  a.g = s->g;
  a.tiles = r.tiles;
  a.planes = s->d_planes;
  a.consts = s->d_consts;
  a.num_filters = s->num_filters;
  a.bands = s->d_bands;
  a.weights = s->d_weights;
  a.tile_first = s->d_tile_first;
  a.tile_list = s->d_tile_list;
  a.out = device_out;
  return a;
}

} /* namespace */

AADApiResult AADHip_SpectrogramRun(struct AADHipSpectrogram *s, uint64_t num_rows, const int16_t *device_rows, uint64_t row_pitch,
                                   uint32_t frames, float *device_out)
{
  if (s == nullptr) return AAD_APIRESULT_INVALID_ARGUMENT;
  const uint32_t B = aad::spectrum_bins(s->n_fft);
  const aad::SpectrumRows r = aad::spectrum_rows(num_rows, address(device_rows), row_pitch, frames, address(device_out), s->win, s->hop,
                                                 s->num_filters != 0 ? s->num_filters : B, s->g.tile_frames);
  if (!r.ok) {
    snprintf(s->ctx->last_error, sizeof(s->ctx->last_error),
             "spectrogram run: a null or unaligned pointer, %u frames below the window's %u, a row pitch of %llu below the frames, or "
             "%llu rows past 64 bits", frames, s->win, (unsigned long long)row_pitch, (unsigned long long)num_rows);
    return AAD_APIRESULT_INVALID_ARGUMENT;
  }
  DeviceGuard guard(s->ctx);
  if (!guard.ok) return AAD_APIRESULT_NG;
  if (num_rows == 0) return AAD_APIRESULT_OK;
  return launched(s, "run", aad::spectrum::launch(spectrogram_args(s, r, num_rows, device_rows, row_pitch, frames, device_out), s->ctx->stream));
}

AADApiResult AADHip_SpectrogramRunMix(struct AADHipSpectrogram *s, uint64_t num_rows, const int16_t *device_rows_a, uint64_t row_pitch_a,
                                      const int16_t *device_rows_b, uint64_t row_pitch_b, uint32_t rows_per_gain, const float *device_gain_a,
                                      const float *device_gain_b, const struct AADHipWindowSpan *device_spans, uint32_t frames,
                                      float *device_out)
{
  if (s == nullptr) return AAD_APIRESULT_INVALID_ARGUMENT;
  const aad::SpectrumRows r = aad::spectrum_mix_rows(num_rows, address(device_rows_a), row_pitch_a, address(device_rows_b), row_pitch_b,
                                                     rows_per_gain, address(device_gain_a), address(device_gain_b), address(device_spans),
                                                     frames, address(device_out), s->win, s->hop,
                                                     s->num_filters != 0 ? s->num_filters : aad::spectrum_bins(s->n_fft), s->g.tile_frames);
  if (!r.ok) {
    snprintf(s->ctx->last_error, sizeof(s->ctx->last_error),
             "spectrogram mix run: a null or unaligned pointer, %u frames below the window's %u, row pitches of %llu and %llu below the "
             "frames, %llu rows past 64 bits or no multiple of %u rows a gain", frames, s->win, (unsigned long long)row_pitch_a,
             (unsigned long long)row_pitch_b, (unsigned long long)num_rows, rows_per_gain);
    return AAD_APIRESULT_INVALID_ARGUMENT;
  }
  DeviceGuard guard(s->ctx);
  if (!guard.ok) return AAD_APIRESULT_NG;
  if (num_rows == 0) return AAD_APIRESULT_OK;
  static_assert(sizeof(AADHipWindowSpan) == 2 * sizeof(uint64_t), "span record layout");
  aad::spectrum_mix::Args m = {};
  m.s = spectrogram_args(s, r, num_rows, device_rows_a, row_pitch_a, frames, device_out);
  m.rows_b = device_rows_b;
  m.row_pitch_b = row_pitch_b;
  m.rows_per_gain = rows_per_gain;
  m.gain_a = device_gain_a;
  m.gain_b = device_gain_b;
  m.spans = reinterpret_cast<const uint64_t *>(device_spans);
  return launched(s, "mix run", aad::spectrum_mix::launch(m, s->ctx->stream));
}
