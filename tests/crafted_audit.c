/* crafted_audit.c - an instrumented restatement of the encoder's block chain WITHOUT the trial search, for
 * tests/test_crafted_pcm.py: it steps aado_encode_step (oracle/aad_oracle.h) sample by sample, restates the block header's weight
 * shift and mask and the code packing around it, and reads the lane before and after every step to count the corners a stream
 * reaches.  The image it writes must equal oracle_binding.encode's (the test checks that first), so the counts describe the
 * recurrence the oracle - and through it the compiled reference - runs.  TEST INFRASTRUCTURE ONLY; built by the test with the
 * oracle's source. */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "../oracle/aad_oracle.h"

enum { /* per-channel record, int64 each */
  AUDIT_STEPS,        /* encoder steps taken (padding samples of a last unit included) */
  AUDIT_CLIP_HI,      /* steps whose reconstruction qd + p was clipped to +32767 */
  AUDIT_CLIP_LO,      /* ... to -32768 */
  AUDIT_IDX_0,        /* steps that began with the step index at 0 */
  AUDIT_IDX_MAX,      /* ... at 4080 */
  AUDIT_MAX_ABS_W,    /* largest |w| seen after any step */
  AUDIT_MAX_SHIFT,    /* largest block-header weight shift */
  AUDIT_SUM_WRAPS,    /* steps whose exact 16384 + sum h*w is not its int32 wrap */
  AUDIT_SQUARE_WRAPS, /* steps whose qd*qd leaves int32 (the trial search's RMSE would wrap it) */
  AUDIT_MAX_ABS_D,    /* largest |x - p| */
  AUDIT_FIELDS
};

static int32_t clip16(int32_t v) { return v < -32768 ? -32768 : v > 32767 ? 32767 : v; }

static uint8_t *put_be(uint8_t *p, uint32_t v, int bytes)
{
  for (int i = bytes - 1; i >= 0; i--) *p++ = (uint8_t)(v >> (8 * i));
  return p;
}

static uint32_t audited_step(AadoLane *l, int32_t x, uint32_t bits, int64_t *a)
{
  int64_t exact = 16384;
  for (int i = 0; i < AADO_TAPS; i++) exact += (int64_t)l->h[i] * (int64_t)l->w[i];
  const int32_t wrapped = (int32_t)(uint32_t)(uint64_t)exact;
  const int32_t p = wrapped >> 15;
  const int64_t d = (int64_t)x - p;
  a[AUDIT_STEPS]++;
  if (exact != (int64_t)wrapped) a[AUDIT_SUM_WRAPS]++;
  if (l->idx == 0) a[AUDIT_IDX_0]++;
  if (l->idx == 4080) a[AUDIT_IDX_MAX]++;
  if ((d < 0 ? -d : d) > a[AUDIT_MAX_ABS_D]) a[AUDIT_MAX_ABS_D] = d < 0 ? -d : d;
  const uint32_t code = aado_encode_step(l, x, bits);
  const int64_t y = (int64_t)l->qerr + p; /* what the step clipped into h[0] */
  if (y > 32767) a[AUDIT_CLIP_HI]++;
  if (y < -32768) a[AUDIT_CLIP_LO]++;
  if ((int64_t)l->qerr * l->qerr > INT32_MAX) a[AUDIT_SQUARE_WRAPS]++;
  for (int i = 0; i < AADO_TAPS; i++) {
    const int64_t w = l->w[i] < 0 ? -(int64_t)l->w[i] : l->w[i];
    if (w > a[AUDIT_MAX_ABS_W]) a[AUDIT_MAX_ABS_W] = w;
  }
  return code;
}

/* pcm: interleaved int16; out: the .aad image; audit: channels x AUDIT_FIELDS int64, zeroed here.  Returns an AADO_* code. */
int crafted_audit_encode(const int16_t *pcm, uint32_t num_samples, uint32_t channels, uint32_t sampling_rate, uint32_t bits,
                         uint32_t max_block_size, uint32_t ms, uint8_t *out, size_t cap, size_t *out_size, int64_t *audit)
{
  AadoHeader hd;
  memset(&hd, 0, sizeof(hd));
  if (channels == 0 || channels > AADO_MAX_CHANNELS || bits < 2 || bits > 4) return AADO_INVALID_FORMAT;
  if (aado_block_geometry(max_block_size, channels, bits, &hd.block_size, &hd.samples_per_block) != AADO_OK) return AADO_INVALID_FORMAT;
  hd.num_channels = channels;
  hd.num_samples = num_samples;
  hd.sampling_rate = sampling_rate;
  hd.bits_per_sample = bits;
  hd.ch_process_method = ms;
  if (cap < aado_encoded_size(num_samples, channels, bits, max_block_size)) return AADO_INSUFFICIENT_BUFFER;
  int rc = aado_put_header(&hd, out, cap);
  if (rc != AADO_OK) return rc;
  memset(audit, 0, sizeof(int64_t) * AUDIT_FIELDS * channels);

  const uint32_t unit_samples = bits == 3 ? 8 : bits == 4 ? 2 : 4, unit_bytes = bits == 3 ? 3 : 1;
  const uint32_t spb = hd.samples_per_block;
  AadoLane lanes[AADO_MAX_CHANNELS];
  memset(lanes, 0, sizeof(lanes));
  int32_t *x = (int32_t *)malloc(sizeof(int32_t) * (size_t)channels * (spb + 8));
  if (!x) return AADO_NG;
  uint8_t *p = out + AADO_FILE_HEADER_BYTES;
  for (uint32_t progress = 0; progress < num_samples;) {
    const uint32_t n = num_samples - progress < spb ? num_samples - progress : spb;
    for (uint32_t s = 0; s < spb + 8; s++) { /* the block's samples, planar, zero past its end; L/R -> M/S per sample */
      for (uint32_t c = 0; c < channels; c++) x[c * (spb + 8) + s] = s < n ? pcm[(size_t)(progress + s) * channels + c] : 0;
      if (ms && channels >= 2 && s < n) {
        const int32_t l = x[s], r = x[(spb + 8) + s];
        x[s] = clip16((l + r) >> 1);
        x[(spb + 8) + s] = clip16((l - r) >> 1);
      }
    }
    for (uint32_t c = 0; c < channels; c++) { /* block header: history, weight shift, masked weights */
      AadoLane *l = &lanes[c];
      const int32_t *xc = x + c * (spb + 8);
      for (uint32_t k = 0; k < AADO_TAPS; k++) l->h[AADO_TAPS - 1 - k] = xc[k];
      int64_t maxabs = 0;
      for (int k = 0; k < AADO_TAPS; k++) {
        /* |INT32_MIN| stays negative in the reference's int32 and so never raises the shift: the same here */
        const int32_t a = l->w[k] >= 0 ? l->w[k] : (int32_t)(0u - (uint32_t)l->w[k]);
        if (maxabs < a) maxabs = a;
      }
      uint32_t shift = 0;
      for (; maxabs > 32767; maxabs >>= 1) shift++;
      if ((int64_t)shift > audit[c * AUDIT_FIELDS + AUDIT_MAX_SHIFT]) audit[c * AUDIT_FIELDS + AUDIT_MAX_SHIFT] = shift;
      for (int k = 0; k < AADO_TAPS; k++) l->w[k] &= (int32_t)~((1u << shift) - 1u);
      p = put_be(p, (((uint32_t)l->idx << 4) & 0xFFFFu) | (shift & 0xFu), 2);
      for (int k = 0; k < AADO_TAPS; k++) {
        p = put_be(p, (uint32_t)(l->w[k] >> shift) & 0xFFFFu, 2);
        p = put_be(p, (uint32_t)l->h[k] & 0xFFFFu, 2);
      }
    }
    for (uint32_t s = AADO_TAPS; s < n; s += unit_samples) {
      for (uint32_t c = 0; c < channels; c++) {
        uint32_t acc = 0;
        for (uint32_t k = 0; k < unit_samples; k++)
          acc = (acc << bits) | audited_step(&lanes[c], x[c * (spb + 8) + s + k], bits, audit + c * AUDIT_FIELDS);
        p = put_be(p, acc, (int)unit_bytes);
      }
    }
    progress += n;
  }
  free(x);
  *out_size = (size_t)(p - out);
  return AADO_OK;
}
