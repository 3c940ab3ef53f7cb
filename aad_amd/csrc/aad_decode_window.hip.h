/*
 * aad_decode_window.hip.h - window decode (AADHip_WindowDecodePlanRun): sample-accurate crops of many streams, straight into
 * planar [windows, channels, frames] rows of int16, float32, float16 or bfloat16.
 *
 * Every block header carries the decoder's whole state (reference src/aad_decoder.c:364-380), so the frames of a crop come from the
 * blocks that cover it alone.  One lane per (window, block-in-window, channel): a window of T frames touches at most
 * K = ceil((T - 1) / spb) + 1 blocks (aad_launch_policy.h window_blocks_spanned), lane k of a window decodes block
 * first_frame / spb + k of its stream and the lanes past the window's own last block idle.  A lane decodes its block from the
 * header on - the samples in front of the crop carry the state - with the per-lane dense decoder's pieces (aad_decode.hip.h: header
 * parse, code fetch one chunk ahead, decode_chunk16, byte-load tail, M/S finish through pair_swap), stops after the last sample the
 * window needs, and stores only the samples inside the window: whole 16-sample chunks as 16-byte vectors at the row's own
 * (2- or 4-byte) alignment, the head and tail of a row sample by sample.  The float16 and bfloat16 rows are the float32 value
 * rounded to nearest even, two samples per v_cvt_pk_f16_f32 / v_cvt_pk_bf16_f32, and leave by the int16 row's stores.  Frames the
 * stream does not produce (past num_samples, past the bytes that are there, a stream index out of range) are written as zeros by
 * the lane whose block holds them.
 *
 * Reads: the 18-byte channel headers only when that many bytes are present, chunk loads only while they lie inside the stream's
 * bytes, the tail byte by byte against the same bound - exactly decode_blocks_kernel's `avail` rule, so no byte outside
 * [data_offset, data_offset + data_size) is read and a truncated image decodes as under AADHip_DecodePlanRun.
 */
#ifndef AAD_DECODE_WINDOW_HIP_H
#define AAD_DECODE_WINDOW_HIP_H

#include "aad_decode.hip.h"
#include "aad_launch_policy.h" /* StreamFormat */
#include "aad_window_span.h"

namespace aad {

struct WindowArgs {
  const StreamDesc *streams;
  const uint8_t *data;
  const uint64_t *windows; /* [num_windows][2]: stream, first_frame (struct AADHipWindow) */
  void *out;               /* [num_windows][channels][frames] of the sample type */
  uint64_t lanes;          /* num_windows * blocks_per_window * channels */
  uint32_t blocks_per_window;
  uint32_t frames;
  uint32_t num_streams;
  uint32_t channels;
  uint32_t block_size;
  uint32_t samples_per_block;
  uint32_t header_bytes; /* 31 (file image) or 0 (bare block) */
  uint32_t mid_side;
  uint32_t bits;
  uint32_t reserved;
};

typedef float f32x4_u4 __attribute__((ext_vector_type(4), aligned(4))); /* a 16-byte store at 4-byte alignment */

/* the sample type of the rows, by its number in the C ABI (enum AADHipSampleType) */
enum WindowSample {
  kRowI16 = AAD_HIP_SAMPLE_INT16,
  kRowF32 = AAD_HIP_SAMPLE_FLOAT32,
  kRowF16 = AAD_HIP_SAMPLE_FLOAT16,
  kRowBF16 = AAD_HIP_SAMPLE_BFLOAT16
};

/* two float32 values as one word of two float16 / bfloat16, the first in the low half: round to nearest even in hardware, one
 * v_cvt_pk_f16_f32 / v_cvt_pk_bf16_f32 (the kernels keep 16-bit subnormals: .amdhsa_float_denorm_mode_16_64 3).  With hi = 0 - a
 * single sample - hipcc folds the float16 case and the scale in front of it into v_fma_mixlo_f16: the product in float32, exact,
 * and the same one rounding */
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
template <int ST>
__device__ __forceinline__ uint32_t pack_half2(float lo, float hi)
{
  static_assert(ST == kRowF16 || ST == kRowBF16, "the 2-byte float types");
  if constexpr (ST == kRowF16) return __builtin_bit_cast(uint32_t, f16x2{(_Float16)lo, (_Float16)hi});
  else return __builtin_bit_cast(uint32_t, bf16x2{(__bf16)lo, (__bf16)hi});
}

/* how a lane's samples reach the output's channels (aad_decode_window_channel_mix.hip.h); kMixNone: channel c into row c */
enum WindowMix { kMixNone = 0, kMixTwin = 1 /* mono source, two rows */, kMixDown = 2 /* stereo source, one row */ };

/* the level statistics of a lane's samples inside its window (AADHip_WindowDecodePlanRunStats): 64-bit sums from the first sample
 * on - one 16-sample chunk at full scale is 2^34 in sum_sq, one long block 2^32 in sum_abs.  Empty without STATS. */
template <bool STATS>
struct WindowLevels {
};
template <>
struct WindowLevels<true> {
  uint64_t sum_sq, sum_abs;
  uint32_t max_abs;
  bool store; /* false: a statistics-only run, `row` is not written (uniform over the run) */
};

/* the gain of a lane's window (AADHip_WindowDecodePlanRunGain, aad_decode_window_gain.hip.h).  Empty without GAIN. */
template <bool GAIN>
struct WindowGain {
};
template <>
struct WindowGain<true> {
  float g;  /* device_gain[w], 1 with a null table */
  bool add; /* AAD_HIP_WINDOW_GAIN_ADD: the element becomes old + g * f (uniform over the run) */
};

/* one row segment of a lane: output element t = base + i for sample i of the block, kept where lo <= t < hi.
 * kMixTwin: every store goes to the row `twin` elements on as well.  kMixDown: y is L + R for the float types, (L + R) >> 1 as int16.
 * float16 / bfloat16 rows hold the bits (uint16_t): the float32 value, exact, then the one rounding of the type.
 * STATS: every kept sample is added to the lane's WindowLevels as the int16 value the row holds, zeros() adds nothing.
 * GAIN (the float types): with f the float32 value above, the element becomes p = fl32(g * f), under `add` fl32(old + p) - two
 * roundings, never one fma - and then the one rounding of the type; zeros() writes g * 0 / old + g * 0 likewise.  The twin rows of
 * kMixTwin hold different old values: each is loaded, added and stored on its own.
 * PLACED (a run with spans, aad_decode_window_placed.hip.h): `row` is the row at the span's first element and lo, hi, base are
 * crop indices as ever; fill() writes the +0 of a STORE run outside the span. */
template <int ST, int MIX = kMixNone, bool STATS = false, bool GAIN = false, bool PLACED = false>
struct WindowRow : WindowLevels<STATS>, WindowGain<GAIN> {
  static_assert(ST == kRowI16 || ST == kRowF32 || ST == kRowF16 || ST == kRowBF16, "a sample type of window decode");
  static_assert(!GAIN || (ST != kRowI16 && !STATS), "a gain is for float rows, and has no statistics variant");
  static_assert(!PLACED || GAIN || STATS, "spans come with a gain run's rows or with a statistics-only run");
  static constexpr bool F32 = ST == kRowF32, HALF = ST == kRowF16 || ST == kRowBF16;
  using T = std::conditional_t<F32, float, std::conditional_t<HALF, uint16_t, int16_t>>;
  T *row;
  int64_t base, lo, hi;
  int64_t twin; /* kMixTwin alone */
  /* exact: an int16 (kMixDown: a sum of two, at most 17 bits) times a power of two */
  __device__ __forceinline__ static float scaled(int32_t y)
  {
    return (float)y * (MIX == kMixDown ? 1.0f / 65536.0f : 1.0f / 32768.0f);
  }
  __device__ __forceinline__ static T convert(int32_t y)
  {
    if constexpr (F32) return scaled(y);
    else if constexpr (HALF) return (T)pack_half2<ST>(scaled(y), 0.0f);
    else return (T)y;
  }
  /* GAIN only.  p = fl32(g * f): one multiply that no add may contract into an fma and no float16 pack into a mixed-precision
   * one - the empty asm makes the product a float32 register value of its own */
  __device__ __forceinline__ float gained(float f) const
  {
#pragma clang fp contract(off)
    float p = this->g * f;
    asm("" : "+v"(p));
    return p;
  }
  __device__ __forceinline__ static float sum(float old, float p)
  {
#pragma clang fp contract(off)
    float s = old + p;
    asm("" : "+v"(s));
    return s;
  }
  /* the float32 value of a row element / the element of a float32 value */
  __device__ __forceinline__ static float widen(T e)
  {
    if constexpr (F32) return e;
    else if constexpr (ST == kRowF16) return (float)__builtin_bit_cast(_Float16, e);
    else return __builtin_bit_cast(float, (uint32_t)e << 16);
  }
  __device__ __forceinline__ static T narrow(float v)
  {
    if constexpr (F32) return v;
    else return (T)pack_half2<ST>(v, 0.0f);
  }
  /* element *q from the float32 value f */
  __device__ __forceinline__ void put(T *q, float f) const
  {
    const float p = gained(f);
    *q = narrow(this->add ? sum(widen(*q), p) : p);
  }
  /* GAIN only.  The old content of a whole chunk under `add`, as the 16-byte vectors it is loaded in at the row's own alignment
   * (float32: four, the 16-bit types: two; `twin`: the second row's under kMixTwin).  window_lane fetches it in front of the
   * chunk's decode, so the loads are in flight while the lane decodes, and hands it to chunk() */
  struct Old {
    static constexpr int NV = F32 ? 4 : 2, PER = kChunk / NV; /* vectors of a chunk, elements of a vector */
    u32x4 v[NV];
    u32x4 twin[MIX == kMixTwin ? NV : 1];
  };
  __device__ __forceinline__ bool whole(int64_t t0) const { return t0 >= lo && t0 + kChunk <= hi; }
  __device__ __forceinline__ void fetch(uint32_t i0, Old &o) const
  {
    const int64_t t0 = base + (int64_t)i0;
    if (!this->add || !whole(t0)) return;
    const T *p = row + t0;
#pragma unroll
    for (int q = 0; q < Old::NV; q++) {
      o.v[q] = reinterpret_cast<const U32x4 *>(p + Old::PER * q)->v;
      if constexpr (MIX == kMixTwin) o.twin[q] = reinterpret_cast<const U32x4 *>(p + twin + Old::PER * q)->v;
    }
  }
  /* 8 elements at q from f[0 .. 7], under `add` on top of the old ones in old[0] (float32: old[0], old[1]): 16-byte stores at the
   * row's own alignment */
  __device__ __forceinline__ void put8(T *q, const float *f, const u32x4 *old) const
  {
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; j++) v[j] = gained(f[j]);
    if constexpr (F32) {
      if (this->add) {
#pragma unroll
        for (int j = 0; j < 8; j++) v[j] = sum(__builtin_bit_cast(float, (uint32_t)old[j / 4][j % 4]), v[j]);
      }
#pragma unroll
      for (int h = 0; h < 2; h++)
        *reinterpret_cast<f32x4_u4 *>(q + 4 * h) = f32x4_u4{v[4 * h], v[4 * h + 1], v[4 * h + 2], v[4 * h + 3]};
    } else {
      if (this->add) {
#pragma unroll
        for (int j = 0; j < 4; j++) {
          v[2 * j] = sum(widen((T)(old[0][j] & 0xFFFFu)), v[2 * j]);
          v[2 * j + 1] = sum(widen((T)(old[0][j] >> 16)), v[2 * j + 1]);
        }
      }
      store_u32x4<false>(reinterpret_cast<int16_t *>(q), u32x4{pack_half2<ST>(v[0], v[1]), pack_half2<ST>(v[2], v[3]),
                                                               pack_half2<ST>(v[4], v[5]), pack_half2<ST>(v[6], v[7])});
    }
  }
  /* STATS only.  The float down-mix carries L + R: its statistic is the int16 floor mix's */
  __device__ __forceinline__ void level(int32_t y)
  {
    const int32_t v = ST != kRowI16 && MIX == kMixDown ? y >> 1 : y;
    const uint32_t m = (uint32_t)(v < 0 ? -v : v); /* at most 32768 */
    this->sum_sq += (uint64_t)m * m;
    this->sum_abs += m;
    this->max_abs = m > this->max_abs ? m : this->max_abs;
  }
  __device__ __forceinline__ bool stores() const
  {
    if constexpr (STATS) return this->store;
    else return true;
  }
  __device__ __forceinline__ void one(uint32_t i, int32_t y)
  {
    const int64_t t = base + (int64_t)i;
    if (t >= lo && t < hi) {
      if constexpr (GAIN) {
        put(row + t, scaled(y));
        if constexpr (MIX == kMixTwin) put(row + t + twin, scaled(y));
      } else if (stores()) {
        row[t] = convert(y);
        if constexpr (MIX == kMixTwin) row[t + twin] = convert(y);
      }
      if constexpr (STATS) level(y);
    }
  }
  /* samples i0 .. i0 + 15; GAIN: old = what fetch(i0, ...) loaded */
  __device__ __forceinline__ void chunk(uint32_t i0, const int32_t *y, [[maybe_unused]] const Old *old = nullptr)
  {
    const int64_t t0 = base + (int64_t)i0;
    if (t0 + kChunk <= lo || t0 >= hi) return;
    if (t0 >= lo && t0 + kChunk <= hi) {
      if constexpr (STATS) {
#pragma unroll
        for (int j = 0; j < kChunk; j++) level(y[j]);
        if (!this->store) return;
      }
      T *p = row + t0;
      if constexpr (GAIN) {
        float f[kChunk];
#pragma unroll
        for (int j = 0; j < kChunk; j++) f[j] = scaled(y[j]);
        constexpr int H = Old::NV / 2; /* vectors of 8 elements */
        put8(p, f, old->v);
        put8(p + 8, f + 8, old->v + H);
        if constexpr (MIX == kMixTwin) {
          put8(p + twin, f, old->twin);
          put8(p + twin + 8, f + 8, old->twin + H);
        }
      } else if constexpr (F32) {
#pragma unroll
        for (int q = 0; q < 4; q++) {
          const f32x4_u4 v = f32x4_u4{convert(y[4 * q]), convert(y[4 * q + 1]), convert(y[4 * q + 2]), convert(y[4 * q + 3])};
          *reinterpret_cast<f32x4_u4 *>(p + 4 * q) = v;
          if constexpr (MIX == kMixTwin) *reinterpret_cast<f32x4_u4 *>(p + twin + 4 * q) = v;
        }
      } else if constexpr (HALF) {
        ChunkPcm o;
#pragma unroll
        for (int h = 0; h < 2; h++)
          o.v[h] = u32x4{pack_half2<ST>(scaled(y[8 * h]), scaled(y[8 * h + 1])),
                         pack_half2<ST>(scaled(y[8 * h + 2]), scaled(y[8 * h + 3])),
                         pack_half2<ST>(scaled(y[8 * h + 4]), scaled(y[8 * h + 5])),
                         pack_half2<ST>(scaled(y[8 * h + 6]), scaled(y[8 * h + 7]))};
        int16_t *h16 = reinterpret_cast<int16_t *>(p); /* the int16 row's stores: 16 bytes at 2-byte alignment */
        store_u32x4<false>(h16, o.v[0]);
        store_u32x4<false>(h16 + 8, o.v[1]);
        if constexpr (MIX == kMixTwin) {
          store_u32x4<false>(h16 + twin, o.v[0]);
          store_u32x4<false>(h16 + twin + 8, o.v[1]);
        }
      } else {
        const ChunkPcm o = pack_chunk_pcm<1, false>(y, 0);
        store_u32x4<false>(p, o.v[0]);
        store_u32x4<false>(p + 8, o.v[1]);
        if constexpr (MIX == kMixTwin) {
          store_u32x4<false>(p + twin, o.v[0]);
          store_u32x4<false>(p + twin + 8, o.v[1]);
        }
      }
      return;
    }
#pragma unroll
    for (int j = 0; j < kChunk; j++) one(i0 + (uint32_t)j, y[j]);
  }
  /* PLACED only.  +0 into elements [from, to) of the whole row `r` (kMixTwin: and of the row `pitch` elements on): 16 elements at
   * a time by the chunk path's 16-byte stores at the row's own alignment, the rest one by one */
  __device__ __forceinline__ static void fill(T *r, int64_t from, int64_t to, [[maybe_unused]] int64_t pitch)
  {
    int64_t t = from;
    for (; t + kChunk <= to; t += kChunk) {
#pragma unroll
      for (int twin = 0; twin < (MIX == kMixTwin ? 2 : 1); twin++) {
        T *p = r + t + twin * pitch;
        if constexpr (F32) {
#pragma unroll
          for (int q = 0; q < 4; q++) *reinterpret_cast<f32x4_u4 *>(p + 4 * q) = f32x4_u4{0.0f, 0.0f, 0.0f, 0.0f};
        } else {
          store_u32x4<false>(reinterpret_cast<int16_t *>(p), u32x4{0, 0, 0, 0});
          store_u32x4<false>(reinterpret_cast<int16_t *>(p) + 8, u32x4{0, 0, 0, 0});
        }
      }
    }
    for (; t < to; t++) {
      r[t] = (T)0;
      if constexpr (MIX == kMixTwin) r[t + pitch] = (T)0;
    }
  }
  /* zeros over [from, hi) */
  __device__ __forceinline__ void zeros(int64_t from) const
  {
    if (!stores()) return;
    for (int64_t t = from > lo ? from : lo; t < hi; t++) {
      if constexpr (GAIN) {
        put(row + t, 0.0f);
        if constexpr (MIX == kMixTwin) put(row + t + twin, 0.0f);
      } else {
        row[t] = (T)0;
        if constexpr (MIX == kMixTwin) row[t + twin] = (T)0;
      }
    }
  }
};

/* CHF: 1 / 2 = the mono / stereo fast paths (wide chunk loads), 0 = any channel count (byte loads).
 * MIXED (aad_decode_window_mixed.hip.h): the block geometry comes from the stream's record in `formats`, not from the launch, and
 * the lane leaves when its stream belongs to another kernel variant - a decision per window, so the lanes of a channel pair take
 * it together.  Windows whose stream is out of range are written (as zeros) by the launch that `owns_strays`.
 * OUTC (aad_decode_window_channel_mix.hip.h; 0: as many as the source has): the rows a window has in the output.  The lanes, the
 * block geometry and every read stay the SOURCE's (CHF); a mono source stores into both rows, a stereo pair exchanges the finished
 * L / R samples once more and lane c == 0 stores the mix into the one row.
 * STATS (aad_decode_window_stats.hip.h): the lane also sums the levels of the samples it keeps and ends by adding them into its
 * row's record of `stats`, which the run cleared; a.out may then be null - nothing is stored, the ranges stay.
 * GAIN (aad_decode_window_gain.hip.h): the lane reads its window's gain from `gain` (null: 1) and its row writer stores g * f, or
 * with `add` adds it to what the row holds (WindowRow).
 * PLACED (aad_decode_window_placed.hip.h; with GAIN, or with STATS and no rows): the window's record of `spans` - (L, o), null:
 * (T, 0) - clips to Le frames (aad_window_span.h) and the lane's crop arithmetic runs over Le instead of T: the early leave, hi,
 * n, count.  The row starts at element o, its pitch stays T.  Under STORE the lane first writes +0 into its fill tile, the part
 * outside the span of the tile it owns in a run without spans - also the lanes that then leave; the R lane of a down-mixed pair
 * fills nothing, a twin fills both rows.  Under ADD nothing outside the span is read or written. */
template <int BITS, int CHF, bool MS, int ST, bool MIXED = false, int OUTC = 0, class FORMAT = StreamFormat, bool STATS = false,
          bool GAIN = false, bool PLACED = false>
__device__ __forceinline__ void window_lane(const WindowArgs &a, const char *lds, uint64_t lane, const FORMAT *formats = nullptr,
                                            uint32_t owns_strays = 0, unsigned long long *stats = nullptr,
                                            const float *gain = nullptr, uint32_t add = 0,
                                            [[maybe_unused]] const uint64_t *spans = nullptr)
{
  static_assert(OUTC == 0 || ((CHF == 1 || CHF == 2) && (OUTC == 1 || OUTC == 2)), "a channel mix is between one and two channels");
  constexpr int MIX = OUTC == 0 || OUTC == CHF ? kMixNone : OUTC == 2 ? kMixTwin : kMixDown;
  const uint32_t ch = CHF ? CHF : a.channels;
  const uint64_t per_window = (uint64_t)a.blocks_per_window * ch;
  const uint64_t w = lane / per_window;
  const uint32_t r = (uint32_t)(lane - w * per_window);
  const uint32_t k = r / ch, c = r - k * ch;
  const uint64_t stream = a.windows[2 * w], first_frame = a.windows[2 * w + 1];
  uint64_t spb = a.samples_per_block;
  uint32_t block_size = a.block_size;
  if constexpr (MIXED) {
    if (stream < a.num_streams) {
      const FORMAT f = formats[stream];
      if constexpr (std::is_same_v<FORMAT, StreamFormat>) {
        if (f.bits != BITS || (f.mid_side != 0) != MS) return;
      } else {
        if (f.bits != BITS || f.source != (CHF == 1 ? kSourceMono : MS ? kSourceMidSide : kSourceStereo)) return;
      }
      spb = f.samples_per_block;
      block_size = f.block_size;
    } else if (!owns_strays) {
      return;
    }
  }
  [[maybe_unused]] const uint64_t pitch = a.frames; /* elements of a row */
  [[maybe_unused]] uint64_t out_frame = 0;
  uint64_t crop = a.frames;
  if constexpr (PLACED) {
    if (spans != nullptr) {
      out_frame = spans[2 * w + 1];
      crop = window_span_frames(spans[2 * w], out_frame, a.frames);
    }
  }
  const uint64_t frames = crop; /* the frames of the crop: T, PLACED: Le */
  const uint64_t phase = first_frame % spb;
  const uint64_t kspb = (uint64_t)k * spb;
  using Row = WindowRow<ST, MIX, STATS, GAIN, PLACED>;
  if constexpr (PLACED && GAIN) {
    if (!add && !(MIX == kMixDown && c)) {
      typename Row::T *r = reinterpret_cast<typename Row::T *>(a.out) + (MIX == kMixNone ? w * ch + c : w * OUTC) * pitch;
      const WindowFillTile tile = window_fill_tile(k, spb, phase, a.frames, out_frame, frames);
      Row::fill(r, tile.lo[0], tile.hi[0], (int64_t)pitch);
      Row::fill(r, tile.lo[1], tile.hi[1], (int64_t)pitch);
    }
  }
  if constexpr (PLACED)
    if (frames == 0) return; /* an empty span: nothing to decode, whatever the phase */
  if (kspb >= frames + phase) return; /* past the window's last block: lanes of one (window, block) leave together */

  Row out;
  if constexpr (STATS) {
    out.sum_sq = out.sum_abs = 0;
    out.max_abs = 0;
    out.store = a.out != nullptr;
  }
  if constexpr (GAIN) {
    out.g = gain != nullptr ? gain[w] : 1.0f;
    out.add = add != 0;
  }
  if constexpr (PLACED) {
    /* frames = Le > 0 here: out_frame < T.  The crop range is aad_window_span.h's */
    out.row = reinterpret_cast<typename Row::T *>(a.out) + (MIX == kMixNone ? w * ch + c : w * OUTC) * pitch + out_frame;
    if constexpr (MIX != kMixNone) out.twin = (int64_t)pitch;
    const WindowCropRange range = window_crop_range(k, spb, phase, frames);
    out.base = range.base;
    out.lo = range.lo;
    out.hi = range.hi;
  } else {
    if constexpr (MIX == kMixNone) {
      out.row = reinterpret_cast<typename WindowRow<ST>::T *>(a.out) + (w * ch + c) * frames;
    } else {
      out.row = reinterpret_cast<typename WindowRow<ST>::T *>(a.out) + w * OUTC * frames;
      out.twin = (int64_t)frames;
    }
    out.base = (int64_t)kspb - (int64_t)phase;
    out.lo = out.base > 0 ? out.base : 0;
    out.hi = out.base + (int64_t)spb < (int64_t)frames ? out.base + (int64_t)spb : (int64_t)frames;
  }

  /* samples of this block the window needs, as far as the stream has them (n = 0: none) */
  uint32_t n = 0, avail = 0;
  [[maybe_unused]] uint64_t count = 0; /* STATS: frames of the window the stream's table has, from the lane of the window's first block */
  const uint8_t *src = a.data;
  if (stream < a.num_streams) {
    const StreamDesc sd = a.streams[stream];
    if (first_frame < sd.num_samples) {
      if constexpr (STATS)
        if (k == 0) count = sd.num_samples - first_frame < frames ? sd.num_samples - first_frame : frames;
      const uint64_t b = first_frame / spb + k;
      const uint64_t first = b * spb;
      if (first < sd.num_samples) {
        const uint64_t left = sd.num_samples - first, need = (uint64_t)(out.hi - out.base);
        n = (uint32_t)(left < need ? left : need);
      }
      /* bytes of this stream still present from the start of this block */
      const uint64_t block_off = a.header_bytes + b * block_size;
      const uint64_t avail64 = sd.data_size > block_off ? sd.data_size - block_off : 0;
      avail = avail64 > 0x7FFFFFFFu ? 0x7FFFFFFFu : (uint32_t)avail64;
      src = a.data + sd.data_offset + block_off;
      if (avail < (uint32_t)kBlockHeaderBytesPerCh * ch) n = 0; /* DecodeBlock: INSUFFICIENT_DATA */
    }
  }

  /* the R lane of a down-mixed pair decodes and exchanges, and stores nothing (`n` above came from the segment both lanes share) */
  if constexpr (MIX == kMixDown)
    if (c) out.lo = out.hi = INT64_MIN;

  Lane L = {0, 0, 0, 0, 0, 0, 0, 0, kIdxBias};
  if (n) { /* block header - reference src/aad_decoder.c:364-380 */
    const uint8_t *hp = src + c * kBlockHeaderBytesPerCh;
    const uint32_t v = load_be16(hp);
    L.idxb = min((int32_t)(v >> 4), (int32_t)kHeaderIdxMax) + kIdxBias;
    const uint32_t shift = v & 0xFu;
    L.w0 = (int32_t)((uint32_t)(int32_t)(int16_t)load_be16(hp + 2) << shift);
    L.h0 = (int16_t)load_be16(hp + 4);
    L.w1 = (int32_t)((uint32_t)(int32_t)(int16_t)load_be16(hp + 6) << shift);
    L.h1 = (int16_t)load_be16(hp + 8);
    L.w2 = (int32_t)((uint32_t)(int32_t)(int16_t)load_be16(hp + 10) << shift);
    L.h2 = (int16_t)load_be16(hp + 12);
    L.w3 = (int32_t)((uint32_t)(int32_t)(int16_t)load_be16(hp + 14) << shift);
    L.h3 = (int16_t)load_be16(hp + 16);
  }

  /* inverse mid/side: the partner channel is the neighbouring lane, of the same window and block, with the same trip counts */
  auto finish = [&](int32_t y) -> int32_t {
    if constexpr (MIX == kMixDown) {
      /* the mix is taken on the finished samples: with mid/side L = clip16(M + S) and R = clip16(M - S), both from the one
       * exchange; right on lane c == 0, which alone stores */
      const int32_t other = (int32_t)pair_swap<false>((uint32_t)y, c);
      const int32_t sum = MS ? clip16(y + other) + clip16(y - other) : y + other;
      return ST != kRowI16 ? sum : sum >> 1; /* the float types keep the half step (WindowRow::scaled), int16 is the floor */
    } else {
      if (MS) {
        const int32_t other = (int32_t)pair_swap<false>((uint32_t)y, c);
        return c == 0 ? clip16(y + other) : clip16(other - y);
      }
      return y;
    }
  };

  constexpr int US = Pack<BITS>::kUnitSamples, UB = Pack<BITS>::kUnitBytes;
  const uint32_t coded = n > (uint32_t)kTaps ? n - kTaps : 0;
  uint32_t done = 0;

  /* the first four samples are stored verbatim in the header - reference :386-391 */
  {
    const int32_t y0 = finish(L.h3), y1 = finish(L.h2), y2 = finish(L.h1), y3 = finish(L.h0);
    if (n > 0) out.one(0, y0);
    if (n > 1) out.one(1, y1);
    if (n > 2) out.one(2, y2);
    if (n > 3) out.one(3, y3);
  }

  if constexpr (CHF != 0) {
    /* full 16-sample chunks whose wide load stays inside the stream's bytes, fetched one chunk ahead */
    using CC = ChunkCodes<BITS, (CHF ? CHF : 1)>;
    constexpr uint32_t kStride = Pack<BITS>::kChunkBytes * (CHF ? CHF : 1);
    const uint32_t body = (uint32_t)kBlockHeaderBytesPerCh * ch;
    uint32_t full = coded / kChunk;
    if (avail < body + CC::kLoadBytes) {
      full = 0;
    } else {
      const uint32_t fit = (avail - body - CC::kLoadBytes) / kStride + 1;
      full = full < fit ? full : fit;
    }
    const uint8_t *cp = src + body;
    CC next;
    next.r[0] = next.r[1] = next.r[2] = next.r[3] = 0;
    if (full) next.load(cp);
    next.touch();
    for (uint32_t q = 0; q < full; q++) {
      uint32_t wd[2] = {0, 0};
      next.unpack(c, wd);
      if (q + 1 < full) cp += kStride; /* unconditional prefetch: the last iteration re-reads its own chunk */
      next.load(cp);
      int32_t y[kChunk];
      if constexpr (GAIN) {
        typename Row::Old old = {};
        out.fetch((uint32_t)kTaps + q * kChunk, old);
        decode_chunk16<BITS>(L, wd, lds, y, finish);
        next.touch();
        out.chunk((uint32_t)kTaps + q * kChunk, y, &old);
      } else {
        decode_chunk16<BITS>(L, wd, lds, y, finish);
        next.touch();
        out.chunk((uint32_t)kTaps + q * kChunk, y);
      }
    }
    done = full * kChunk;
  } else {
    /* any channel count: the units of a channel are UB * channels bytes apart (byte loads) */
    using CA = ChunkCodesAny<BITS>;
    const uint32_t body = (uint32_t)kBlockHeaderBytesPerCh * ch;
    const uint32_t unit_stride = UB * ch, row = CA::kUnits * unit_stride;
    uint32_t full = coded / kChunk;
    const uint32_t fit = avail > body ? (avail - body) / row : 0u;
    full = full < fit ? full : fit;
    const uint8_t *cp = src + body + c * UB;
    CA next;
    for (auto &v : next.b) v = 0;
    if (full) next.load(cp, unit_stride);
    next.touch();
    for (uint32_t q = 0; q < full; q++) {
      uint32_t wd[2] = {0, 0};
      next.unpack(wd);
      if (q + 1 < full) cp += row;
      next.load(cp, unit_stride);
      int32_t y[kChunk];
      if constexpr (GAIN) {
        typename Row::Old old = {};
        out.fetch((uint32_t)kTaps + q * kChunk, old);
        decode_chunk16<BITS>(L, wd, lds, y, finish);
        next.touch();
        out.chunk((uint32_t)kTaps + q * kChunk, y, &old);
      } else {
        decode_chunk16<BITS>(L, wd, lds, y, finish);
        next.touch();
        out.chunk((uint32_t)kTaps + q * kChunk, y);
      }
    }
    done = full * kChunk;
  }

  /* remaining units: byte loads, bytes past the stream read as zero */
  {
    const uint32_t unit_stride = UB * ch;
    const uint32_t base = (uint32_t)kBlockHeaderBytesPerCh * ch + c * UB;
    for (uint32_t i = done; i < coded; i += US) {
      const uint32_t o = base + (i / US) * unit_stride;
      uint32_t acc = 0;
#pragma unroll
      for (int q = 0; q < UB; q++) acc = (acc << 8) | (o + q < avail ? (uint32_t)src[o + q] : 0u);
      acc <<= 32 - 8 * UB; /* codes to the top of the word */
#pragma unroll
      for (int q = 0; q < US; q++) {
        const int32_t y = finish(decode_step<BITS>(L, acc >> (32 - BITS), lds));
        acc <<= BITS;
        if (i + q < coded) out.one((uint32_t)kTaps + i + q, y);
      }
    }
  }
  out.zeros(out.base + (int64_t)n);

  if constexpr (STATS) {
    /* the lanes of a row's K blocks meet in its record: integer adds and a max, so any order gives the same bits.  The R lane of a
     * down-mixed pair kept nothing; a lane without a non-zero sample and the records of stray windows leave the cleared zeros */
    if (MIX == kMixDown && c) return;
    unsigned long long *rec = stats + 4 * (MIX == kMixNone ? w * ch + c : w * OUTC);
#pragma unroll
    for (int twin = 0; twin < (MIX == kMixTwin ? 2 : 1); twin++, rec += 4) {
      if (out.sum_abs) {
        atomicAdd(rec, (unsigned long long)out.sum_sq);
        atomicAdd(rec + 1, (unsigned long long)out.sum_abs);
        atomicMax(rec + 2, (unsigned long long)out.max_abs);
      }
      if (count) atomicAdd(rec + 3, (unsigned long long)count);
    }
  }
}

template <int BITS, int CHF, bool MS, int ST>
__global__ void __launch_bounds__(256) decode_window_kernel(WindowArgs a)
{
  __shared__ __attribute__((aligned(16))) char lds[kLdsBytesDenseDec];
  stage_tables<BITS, false>(lds);
  stage_dense_decode_tables<BITS>(lds);
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x; /* a multiple of 64: the lanes of a channel pair stay neighbours */
  for (uint64_t lane = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; lane < a.lanes; lane += stride)
    window_lane<BITS, CHF, MS, ST>(a, lds, lane);
}

} /* namespace aad */

#endif /* AAD_DECODE_WINDOW_HIP_H */
