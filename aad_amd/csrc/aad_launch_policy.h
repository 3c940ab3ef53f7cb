/* aad_launch_policy.h - every launch decision of an encode or decode run (kernel, workgroup, grid, dynamic LDS, scratch), host-only
 * C++17 so that a CPU test pins them (tests/test_launch_policy.py).  Residency terms come from Device (filled once per context),
 * measured crossovers are named constants with their provenance; the engine switches from a plan to a template instantiation. */
#ifndef AAD_LAUNCH_POLICY_H
#define AAD_LAUNCH_POLICY_H

#include <stdint.h>

#include "../../include/aad_hip.h"
#include "aad_lds_layout.h"

namespace aad {

struct Device {
  uint32_t cus, lds_per_cu; /* compute units, LDS bytes per CU */
};

/* AADHip_ContextSetOption's lane mapping and trial lanes, and the measurement aids (read when the context is created) */
struct Knobs {
  int32_t lane_mapping = AAD_HIP_LANE_MAPPING_AUTO;
  int32_t trial_lanes = AAD_HIP_TRIAL_LANES_DUAL;
  int32_t encode_ring = 1;    /* AAD_HIP_ENCODE_RING: 0 never, 1 by policy, 2 every geometry that can */
  int32_t encode_lds_pad = -1; /* AAD_HIP_ENCODE_LDS_PAD bytes; < 0: by policy */
  int32_t decode_lds_pad = -1; /* AAD_HIP_DECODE_LDS_PAD bytes; < 0: by policy */
  uint64_t decode_nt_min = 0;  /* AAD_HIP_DECODE_NT_MIN lanes */
  int32_t simd_role = AAD_HIP_SIMD_ROLE_OFF; /* AAD_HIP_OPTION_SIMD_ROLE: off, or the SIMD (0..3) of the context's busy waves */
};

struct EncodeBatch {
  uint32_t bits, channels, streams, trials, block_size;
  bool ring_ok; /* every image, and the image buffer, on a 64-byte boundary */
};

struct DecodeBatch { /* DecodeArgs' fields of the same names; pcm_base_aligned16: the PCM buffer itself on a 16-byte boundary */
  uint64_t blocks;
  uint32_t streams, channels, bits, samples_per_block, block_size, code_phase_uniform;
  bool pcm_aligned16, pcm_base_aligned16, stream_stores;
};

enum class EncodeKernel { Dense, DenseRing, Quad, QuadDual };
struct EncodeLaunch {
  EncodeKernel kernel;
  bool trials; /* the TRIALS instantiation */
  uint32_t workgroup, grid, lds, trial_slot_bytes;
  uint64_t trial_scratch_bytes; /* 0: none */
  uint32_t simd_role; /* Quad: 0, or 1 + SIMD - four-wave workgroups of sixteen recurrences whose wave on that SIMD works (plan_simd_role) */
};

enum class DecodeKernel { SplitLds, SplitScratch, QuadFused, Tiled, Dense };
struct DecodeLaunch {
  DecodeKernel kernel;
  bool stream_stores; /* Dense: the streamed-store (NT) instantiation */
  uint32_t workgroup, grid, lds, residual_stride;
  uint64_t residual_bytes; /* SplitScratch */
  /* SplitLds / SplitScratch under a role: 1 + SIMD of the recurrence wave, else 0.  SplitLds then keeps its residual rows in
   * dynamic LDS (`lds` bytes, sixteen rows of lds_row dwords sized to the block) */
  uint32_t simd_role, lds_row;
};

constexpr uint32_t kSimdsPerCu = 4, kWaveLanes = 64;

/* threads that put one wave on every SIMD of the chip (65 536 on the MI355X) */
inline uint64_t one_wave_per_simd(const Device &d) { return (uint64_t)d.cus * kSimdsPerCu * kWaveLanes; }

/* Lanes are scarce in every BASELINE config: while the batch has fewer
 * waves than the chip has SIMDs each wave gets a workgroup of its own so the
 * dispatcher spreads them over as many SIMDs as possible; big batches use 256-thread
 * workgroups so four waves share one LDS copy of the tables. */
inline uint32_t pick_workgroup(const Device &d, uint64_t threads) { return threads <= one_wave_per_simd(d) ? 64u : 256u; }

inline uint32_t grid_for(uint64_t threads, uint32_t workgroup) { return (uint32_t)((threads + workgroup - 1) / workgroup); }

/* SIMD roles (AAD_HIP_OPTION_SIMD_ROLE; the election: aad_device.hip.h).  A role applies to the launches that keep ONE wave per
 * workgroup busy - the quad encoder in one-wave workgroups, the split decoder - and only while every workgroup can have a CU of
 * its own: the workgroups of one launch elect the SAME SIMD, so two of them on one CU would share it, where today's one-wave
 * workgroups spread over the CU's SIMDs.  -> 0 (no role), or 1 + SIMD. */
inline uint32_t plan_simd_role(const Device &d, const Knobs &k, uint32_t workgroups)
{
  if (k.simd_role < 0 || k.simd_role >= (int32_t)kSimdsPerCu || workgroups > d.cus) return 0;
  return 1u + (uint32_t)k.simd_role;
}

/* The split decoder's residual rows under a role: the block's coded samples rounded up to a chunk, + 4 dwords (a row length of
 * 4 or 20 mod 32 dwords: the sixteen rows a wave reads at the same sample offset spread over the banks, as kLdsResidualRow's do).
 * Every read of the recurrence wave stays inside: whole chunks up to the rounded length, the tail's one wide load included. */
inline uint32_t split_lds_row(uint32_t coded) { return (coded + (uint32_t)kChunk - 1u) / (uint32_t)kChunk * (uint32_t)kChunk + 4u; }

/* On the quad mapping the trial search's probe strand gets lanes of its own ("dual"): one pass of
 * latency less per block with a predecessor, nothing lost otherwise (tools/trial_probe.py).
 * AAD_HIP_OPTION_TRIAL_LANES = single keeps both strands on the same lanes (the parity tests run both). */
/* Round 4: ... up to kDualMaxRecurrences.  The dual layout spends eight lanes per recurrence; from ~640 waves on (5120 recurrences)
 * its launch slows down faster than the work grows and the one-after-the-other layout - flat up to 16 384 recurrences - overtakes it
 * in every geometry (stereo 4-bit, t = 2: dual 0.146 / 0.161 / 0.231 ms at 4096 / 5120 / 6144 recurrences, single 0.188-0.190;
 * profiles/r04_trial_search_size_sweep.txt). */
constexpr uint64_t kDualMaxRecurrences = 5120;
/* the dual trial search keeps up to two alternative encodes of a block (and what measuring lanes write)
 * beside the image: three slots of one block per stream; beyond this cap the search and the encode run one after the other */
constexpr uint64_t kMaxTrialScratchBytes = 1ull << 30;

/* the dense encoders' static LDS */
template <int BITS>
constexpr uint32_t dense_encoder_lds_of(uint32_t ch) { return ch == 1 ? kLdsBytesEncoder<BITS, 1, false> : ch == 2 ? kLdsBytesEncoder<BITS, 2, false> : kLdsBytesEncoder<BITS, 0, false>; }
inline uint32_t dense_encoder_lds(uint32_t bits, uint32_t ch) { return bits == 4 ? dense_encoder_lds_of<4>(ch) : bits == 3 ? dense_encoder_lds_of<3>(ch) : dense_encoder_lds_of<2>(ch); }

/* One-wave workgroups (pick_workgroup: up to one wave per SIMD) only while ALL of them can be resident at once: a dense mono encoder
 * holds 45-52 KB of LDS per workgroup (wide table + code staging or ring rows), so a CU takes three of them and its fourth SIMD
 * stays empty - from 49 153 lanes (769 waves) on the launch ran in two rounds (mono 4-bit, 64 000 one-block streams: 0.35-0.41 ms
 * against 0.19 ms for 48 000, profiles/r04_encoder_ring_midsize.txt).  Four-wave workgroups share one table: two per CU. */
inline uint32_t dense_encode_workgroup(const Device &d, uint64_t lanes, uint32_t lds_one_wave)
{
  const uint32_t wg = pick_workgroup(d, lanes);
  if (wg != 64u) return wg;
  const uint64_t waves = (lanes + 63u) / 64u;
  const uint64_t resident = (uint64_t)d.cus * (d.lds_per_cu / ((lds_one_wave + 1023u) & ~1023u)); /* CUs x workgroups whose LDS fits */
  return waves > resident ? 256u : 64u;
}

/* Which dense encoders append to the byte ring.  Policy (same-box A/B on the saturated batches, profiles/r03_encoder_byte_ring.txt):
 * every mono encoder and the stereo 4-bit one - their writes fall from 1.3-2.1x to 1.00-1.06x of the code bytes and the kernels
 * get 3-8 % faster; stereo 3- and 2-bit - no: they are VALU-saturated (95 % active), wrote only 1.18x in total before, and the
 * ring's extra ~1 VALU instruction per sample costs them 3-7 % of their time.  AAD_HIP_ENCODE_RING = 0: never (A/B measurements),
 * = 2: every geometry that can.
 * Round 4: only in four-wave workgroups.  Batches of 16 385 .. 65 536 lanes run one-wave workgroups (a wave per SIMD, as many
 * CUs as possible); there the ring is 1-4 % SLOWER than the plain stores (same-box A/B, profiles/r04_encoder_ring_midsize.txt:
 * mono 40 000 streams 0.1835 vs 0.1811 ms, stereo 4-bit 28 000 streams 0.1044 vs 0.1003 ms) - a launch that leaves SIMDs idle
 * gains nothing from fewer write sectors and pays the ring's instructions on its critical path. */
inline bool encode_ring_wanted(const Knobs &k, uint32_t bits, uint32_t channels, uint32_t workgroup)
{
  if (k.encode_ring != 1) return k.encode_ring == 2;
  return workgroup == 256u && (channels == 1 || bits == 4);
}

/* Occupancy cap of the dense 4-bit encoders on chip-filling batches: unused dynamic LDS up to half the CU's LDS per workgroup, so
 * that a CU holds two workgroups = two waves per SIMD instead of three or four.  These kernels are bound by VALU issue (85 % VALU-
 * active with two waves as with four), but every resident lane keeps one 128-byte line of PCM and one sector of codes alive
 * in the L2 between its visits: 8192 lines per CU at four waves per SIMD - 8 MiB per XCD against 4 MiB of L2 - and a line
 * was fetched 2.2 (mono) / 1.27 (stereo) times; with two waves per SIMD 1.57 / 1.01 times, at the same kernel time
 * (profiles/r03_encoder_occupancy_cap.txt).  The 3- and 2-bit encoders are VALU-saturated (96-103 % active) and lose 4-6 % of
 * their time under the same cap for a similar cut in traffic: they keep their occupancy.  AAD_HIP_ENCODE_LDS_PAD overrides the
 * policy for experiments. */
inline uint32_t dense_encode_lds_pad(const Device &d, const Knobs &k, uint32_t bits, uint64_t lanes, uint32_t static_lds)
{
  if (k.encode_lds_pad >= 0) return (uint32_t)k.encode_lds_pad;
  const uint32_t target = d.lds_per_cu / 2; /* two workgroups per CU */
  if (bits != 4 || lanes < one_wave_per_simd(d) || static_lds >= target) return 0;
  return target - static_lds;
}

/* Lane mapping by batch size.  "quad" (four lanes per recurrence, fewer instructions on the
 * recurrence's critical path) while the batch cannot fill the chip anyway, "dense" (one lane per
 * recurrence, fewest total instructions) beyond; the decoder has the split quad kernel below the
 * fused one.  The crossovers were measured per (bits, channels) geometry on one-block streams
 * (tools/mapping_crossover.py, profiles/r02_mapping_crossover.jsonl): for the encoder it sits where the quad
 * mapping starts to put a second wave on a SIMD (4 x 16384 lanes = one wave on each of the 1024
 * SIMDs).  A context option (AADHip_ContextSetOption, default from
 * AAD_HIP_MAPPING at context creation) forces one mapping; the parity tests run all of them. */
inline EncodeLaunch plan_encode(const Device &d, const Knobs &k, const EncodeBatch &b)
{
  EncodeLaunch p = {};
  const uint64_t lanes = (uint64_t)b.streams * b.channels;
  const int32_t m = b.channels > 2 ? AAD_HIP_LANE_MAPPING_DENSE : k.lane_mapping; /* the quad mapping: mono / stereo */
  const bool quad = m == AAD_HIP_LANE_MAPPING_QUAD || m == AAD_HIP_LANE_MAPPING_QUAD_FUSED || (m == AAD_HIP_LANE_MAPPING_AUTO && lanes <= one_wave_per_simd(d) / 4);
  p.trials = b.trials != 0;
  if (quad && p.trials && k.trial_lanes != AAD_HIP_TRIAL_LANES_SINGLE && lanes <= kDualMaxRecurrences) {
    const uint32_t slot = (b.block_size + 16u + 63u) & ~63u;
    const uint64_t want = (uint64_t)b.streams * 3u * slot;
    if (want <= kMaxTrialScratchBytes) {
      p.trial_slot_bytes = slot;
      p.trial_scratch_bytes = want;
    }
  }
  if (quad) {
    const bool dual = p.trial_scratch_bytes != 0;
    const uint64_t threads = lanes * (dual ? 8 : 4);
    p.kernel = dual ? EncodeKernel::QuadDual : EncodeKernel::Quad;
    /* dual: eight lanes per recurrence put a wave on twice as many CUs as the trial-free launch; two waves
     * per workgroup (two SIMDs of one CU) keep a small batch on half the chip, so that a decode launched
     * beside it finds free CUs (bench.py's pipelined step with trials 2: 158 -> see DESIGN.md)
     * (round 4: two-wave workgroups only while there is at most one of them per CU - 4096 recurrences on the MI355X.  Beyond that a
     * CU receives a second workgroup whose two waves land on the SIMDs the first one's already use, the other two SIMDs stay empty
     * and the launch takes 1.6x as long: stereo 4-bit, t = 2, 6000 recurrences 0.229 ms against 0.143 at 4096;
     * profiles/r04_trial_search_size_sweep.txt.  One-wave workgroups spread over the SIMDs.) */
    p.workgroup = dual && threads <= 128ull * d.cus ? 128u : pick_workgroup(d, threads);
    p.grid = grid_for(threads, p.workgroup);
    if (!dual && p.workgroup == 64u) { /* lane-starved: one wave per sixteen recurrences */
      p.simd_role = plan_simd_role(d, k, p.grid);
      if (p.simd_role) p.workgroup = 256u; /* the same grid: three of a workgroup's four waves only help to stage the tables */
    }
    return p;
  }
  /* the dense encoders, with and without the trial search: one-wave workgroups only while their LDS lets all of them be resident */
  p.kernel = EncodeKernel::Dense;
  uint32_t static_lds = dense_encoder_lds(b.bits, b.channels);
  p.workgroup = dense_encode_workgroup(d, lanes, static_lds);
  p.grid = grid_for(lanes, p.workgroup);
  if (p.trials) return p;
  if (b.ring_ok && b.channels <= 2 && encode_ring_wanted(k, b.bits, b.channels, p.workgroup)) {
    /* the rows' byte rings: dynamic LDS, one wave's worth per wave of the workgroup */
    p.kernel = EncodeKernel::DenseRing;
    p.lds = (p.workgroup / 64u) * (uint32_t)(b.channels == 1 ? kLdsRingBytesPerWave<1> : kLdsRingBytesPerWave<2>);
    static_lds = (uint32_t)kLdsCodeStageOff + p.lds;
  }
  if (p.workgroup == 256u) p.lds += dense_encode_lds_pad(d, k, b.bits, lanes, static_lds);
  return p;
}

/* Planar reconstruct plans (AADHip_PlanarReconstructPlanRun): the encoders whose encode pass also writes the decoded rows.  The
 * trial search always takes the single layout - the dual one encodes every candidate into a slot and moves the winner, so no pass
 * knows its samples are the ones that stay - and no byte ring: the row stores ride the plain chunk loops (aad_encode.hip.h RecRow). */
inline EncodeLaunch plan_reconstruct_encode(const Device &d, const Knobs &k, const EncodeBatch &b)
{
  Knobs r = k;
  r.trial_lanes = AAD_HIP_TRIAL_LANES_SINGLE;
  r.encode_ring = 0;
  return plan_encode(d, r, b);
}

/* The output rows of a planar reconstruct plan (struct AADHipPlanarOutput) for a batch of `channels`-channel streams: false for an
 * unknown sample type, a non-zero reserved, C > 1 with channel_stride below the longest stream, more than one stream with
 * stream_stride below (C - 1) channel_stride + the longest stream (rows of different streams would overlap), or an end of the rows
 * ((N - 1) stream_stride + (C - 1) channel_stride + the longest stream, in elements or in bytes) past 2^64. */
/* planar_output_rows_ok: for num_streams streams whose longest row has `longest` elements (a window reconstruct run: N windows,
 * longest = T); planar_output_ok: for a plan's stream table */
inline bool planar_output_rows_ok(uint32_t channels, uint64_t num_streams, uint64_t longest, const AADHipPlanarOutput *o)
{
  if (o == nullptr || channels == 0) return false;
  if ((o->sample_type != AAD_HIP_SAMPLE_INT16 && o->sample_type != AAD_HIP_SAMPLE_FLOAT32) || o->reserved != 0) return false;
  if (channels > 1 && o->channel_stride < longest) return false;
  uint64_t span = 0; /* elements from a stream's first to past its last */
  if (__builtin_mul_overflow((uint64_t)(channels - 1), o->channel_stride, &span) || __builtin_add_overflow(span, longest, &span)) return false;
  if (num_streams > 1 && o->stream_stride < span) return false;
  const uint64_t elem = o->sample_type == AAD_HIP_SAMPLE_FLOAT32 ? 4u : 2u;
  uint64_t end = 0, bytes = 0;
  if (num_streams != 0 && (__builtin_mul_overflow(num_streams - 1, o->stream_stride, &end) ||
                           __builtin_add_overflow(end, span, &end) || __builtin_mul_overflow(end, elem, &bytes)))
    return false;
  return true;
}
inline bool planar_output_ok(uint32_t channels, uint32_t num_streams, const AADHipStreamDesc *streams, const AADHipPlanarOutput *o)
{
  uint64_t longest = 0;
  for (uint32_t i = 0; i < num_streams; i++) longest = streams[i].num_samples > longest ? streams[i].num_samples : longest;
  return planar_output_rows_ok(channels, num_streams, longest, o);
}

/* Round 4 (tools/size_sweep.py --mapping quad | dense, profiles/r04_decode_split_crossover.txt): the split decoder runs
 * 1024-thread workgroups of 16 recurrences, ONE to a CU (84-94 VGPRs x 16 waves), i.e. rounds of 4096 recurrences: its time is
 * about 0.025 + 0.015 ms x rounds on stereo 4-bit.  Up to two rounds (8192 recurrences) it beats the dense kernel in every
 * geometry (mono 4-bit 0.090 vs 0.116 ms at 8192), from the third round on (9000) it loses in every
 * geometry (0.120 vs 0.116) and its residual scratch (recurrences x block x 4 bytes, ~100 MB at 12 288 mono rows) pushes the
 * NEXT launch's input out of the caches: a mono 4-bit encode behind it took 0.15-0.20 ms instead of 0.127.  Round 2's
 * per-geometry limits (12 288; 9 216 / 8 192 for 4- / 3-bit stereo) predate the dense decoder's round-3 speed-ups.
 * Since the dense decoder's sample went from 32.5 to 24 instructions it is as fast as the fused quad decoder at every batch size
 * (59-60 us on one-block stereo 4-bit streams, 250 to 48 000 recurrences; fused 61-67 us up to 16 384):
 * "auto" never picks the fused kernel, the option still forces it. */
constexpr uint64_t kDecodeSplitMax = 8192;
/* Quad decode runs its two strands on different lanes (aad_decode_split.hip.h) unless
 * AAD_HIP_MAPPING=quad-fused asks for the one-lane-does-both kernel or the residual scratch would be
 * unreasonably large. */
constexpr uint64_t kMaxResidualBytes = 1ull << 30;
/* Dense batches at and beyond this many recurrences take the sector-tiled kernel where it applies (aad_decode_tiled.hip.h).
 * Measured against the per-lane kernel (with its own occupancy cap) on one-block streams, same box, tools/saturated_probe.py
 * (profiles/r03_tiled_decode_crossover.txt): mono 4-bit wins from 65 536 blocks on (one wave per SIMD: 0.156 vs 0.198 ms;
 * 0.43 vs 0.48 ms at 196 608; 1.10 vs 1.29 ms at 524 288), stereo 4-bit from ~393 216 recurrences (0.42 vs 0.45 ms; equal at
 * 262 144, the per-lane kernel ahead below); mono 2-bit like mono 4-bit (2.15 vs 2.52 ms at 524 288 blocks); mono 3-bit (where
 * the batch's layout admits it: aad_decode_tiled.hip.h "3-bit rows") 1.41-1.43 vs 1.70 ms at 524 288 blocks.  On STEREO 2-bit
 * streams the tiled kernel moves 1.02x the algorithmic bytes instead of 1.35x but takes 3-7 % longer (1.04-1.08 vs 1.01-1.02 ms),
 * on stereo 3-bit streams both take 0.73 ms: "auto" keeps the per-lane kernel there, AAD_HIP_LANE_MAPPING_DENSE_TILED selects the
 * tiled one at any size. */
constexpr uint64_t kTiledStereo4Min = 393216;
inline uint64_t tiled_decode_min(const Device &d, uint32_t bits, uint32_t channels)
{
  /* round 4 (tools/size_sweep.py --mapping dense | dense-tiled): at exactly one wave per SIMD of mono lanes the per-lane kernel
   * still runs in one-wave workgroups and is 7 % ahead (65 536: 0.154 vs 0.165 ms); from the next lane on it needs a second wave per
   * SIMD and the tiled kernel is level (80 000) to 18 % ahead (524 288) */
  if (channels == 1) return one_wave_per_simd(d) + 1;
  return bits == 4 ? kTiledStereo4Min : ~0ull;
}

/* true when the batch is small enough, and its blocks short enough, for the split decoder's residuals to stay in LDS */
inline bool decode_split_fits_lds(const Device &d, const DecodeBatch &b)
{
  const uint32_t coded = b.samples_per_block > 4 ? b.samples_per_block - 4 : 0;
  return coded <= kLdsResidualMax && b.blocks * b.channels <= 16ull * d.cus; /* one 16-recurrence workgroup per CU */
}

/* true when decode_tiled_kernel can decode this batch: mono / stereo, 3-bit codes only at a batch-wide code phase, every block's
 * PCM 16-byte aligned */
inline bool decode_tiled_applicable(const DecodeBatch &a)
{
  if (a.channels < 1 || a.channels > 2) return false;
  if (a.bits < 2 || a.bits > 4) return false;
  if (!a.pcm_aligned16 || !a.pcm_base_aligned16) return false;
  /* A block whose header asks for more samples than its block_size holds reads on into the bytes behind it (the reference's
   * code walk has no bound, src/aad_decoder.c:396-451; no encoder writes such a header).  The rows' rings are laid out for
   * blocks that keep to themselves: those streams take the per-lane kernel, which reads through to the end of the stream. */
  const uint64_t us = a.bits == 3 ? 8u : (a.bits == 4 ? 2u : 4u), ub = (uint64_t)(a.bits == 3 ? 3u : 1u) * a.channels;
  const uint64_t coded = a.samples_per_block > 4 ? a.samples_per_block - 4 : 0;
  if ((uint64_t)kBlockHeaderBytesPerCh * a.channels + (coded + us - 1) / us * ub > a.block_size) return false;
  /* every block of a stream starts on a piece boundary: the block length in PCM bytes is a multiple of 16 (mono 2-bit
   * blocks of 1024 bytes hold 4028 samples = 8056 bytes: 8 mod 16, which the kernel takes with a short lead chunk) - or no stream has a second block */
  const uint64_t block_pcm_bytes = (uint64_t)a.samples_per_block * a.channels * 2u;
  const bool odd8_ok = a.bits == 2 && a.channels == 1 && block_pcm_bytes % 16u == 8u; /* DecodeTile::kOdd8: a short lead chunk for every second block */
  if (block_pcm_bytes % 16u != 0 && !odd8_ok && a.blocks > a.streams) return false;
  /* 3-bit rows: the code bytes of every block at the same offset inside their granule (aad_decode_tiled.hip.h "3-bit rows") */
  if (a.bits == 3 && !(a.code_phase_uniform == 1 || (a.code_phase_uniform == 2 && a.blocks <= a.streams))) return false;
  return true;
}

/* Occupancy cap of the per-lane dense decoders on chip-filling batches (what is left to them since the sector-tiled kernel:
 * 3-bit streams, layouts whose PCM is not 16-byte aligned, more than two channels): unused dynamic LDS up to half the CU's LDS per
 * workgroup = two workgroups per CU = two waves per SIMD.  These kernels wait for memory (56-59 % VALU-active on mono 3-bit
 * streams), and what they wait for is lines that were evicted between two visits of the same lane: with fewer lanes resident
 * the L2 keeps more of them.  Mono 3-bit, 524 288 blocks: 2.00 -> 1.72 ms (688 -> 801 Gsamples/s), stereo 3-bit 0.762 -> 0.733 ms;
 * one wave per SIMD is slower again (1.75 / 0.86 ms); profiles/r03_decoder_occupancy_cap.txt.  AAD_HIP_DECODE_LDS_PAD overrides the policy. */
inline uint32_t dense_decode_lds_pad(const Device &d, const Knobs &k, uint64_t lanes, uint32_t channels, uint32_t bits)
{
  if (k.decode_lds_pad >= 0) return (uint32_t)k.decode_lds_pad;
  /* same-box A/B of every geometry on this kernel: mono 4- / 3- / 2-bit +0 / +16 / +7 %, stereo 3- / 2-bit +4 / +2 %, stereo
   * 4-bit (streamed stores) -4 %: that one keeps its occupancy, and so do the any-channel launches (no change) */
  const bool gains = channels == 1 || (channels == 2 && bits != 4);
  return gains && lanes >= one_wave_per_simd(d) ? d.lds_per_cu / 2 - (uint32_t)kLdsBytesDenseDec : 0u;
}

/* Fallbacks: split with the residuals in LDS -> split with a scratch buffer -> (residual scratch over kMaxResidualBytes) the fused
 * quad kernel when the quad mapping is forced, else the per-lane dense one.  Dense: the sector-tiled kernel for chip-filling batches
 * (or when the option asks for it) where it applies, else the per-lane dense kernel. */
inline DecodeLaunch plan_decode(const Device &d, const Knobs &k, const DecodeBatch &b)
{
  DecodeLaunch p = {};
  const uint64_t lanes = b.blocks * b.channels;
  const int32_t m = b.channels > 2 ? AAD_HIP_LANE_MAPPING_DENSE : k.lane_mapping;
  bool quad = m == AAD_HIP_LANE_MAPPING_QUAD_FUSED;
  if (m == AAD_HIP_LANE_MAPPING_QUAD || (m == AAD_HIP_LANE_MAPPING_AUTO && lanes <= kDecodeSplitMax)) {
    /* 64-bit: samples_per_block comes straight from a file header and may be anything */
    const uint64_t coded = b.samples_per_block > 4 ? (uint64_t)b.samples_per_block - 4 : 0;
    const uint64_t row = (coded + 15u) / 16u * 16u + 16u;
    if (row <= kMaxResidualBytes / sizeof(int32_t) && lanes * row * sizeof(int32_t) <= kMaxResidualBytes) {
      p.workgroup = 1024; /* 16 recurrences per workgroup */
      p.grid = grid_for(lanes, 16);
      p.simd_role = plan_simd_role(d, k, p.grid);
      if (decode_split_fits_lds(d, b)) {
        p.kernel = DecodeKernel::SplitLds;
        if (p.simd_role) {
          p.lds_row = split_lds_row((uint32_t)coded);
          p.lds = 16u * p.lds_row * (uint32_t)sizeof(int32_t);
        }
      } else {
        p.kernel = DecodeKernel::SplitScratch;
        p.residual_stride = (uint32_t)row;
        p.residual_bytes = lanes * row * sizeof(int32_t);
      }
      return p;
    }
    quad = m == AAD_HIP_LANE_MAPPING_QUAD;
  } else if (!quad && m != AAD_HIP_LANE_MAPPING_DENSE &&
             (m == AAD_HIP_LANE_MAPPING_DENSE_TILED || lanes >= tiled_decode_min(d, b.bits, b.channels)) && decode_tiled_applicable(b)) {
    p.kernel = DecodeKernel::Tiled;
    p.workgroup = kWaveLanes * kTiledWaves;
    p.grid = grid_for(lanes, p.workgroup);
    return p;
  }
  const uint64_t threads = quad ? lanes * 4 : lanes;
  p.kernel = quad ? DecodeKernel::QuadFused : DecodeKernel::Dense;
  p.workgroup = pick_workgroup(d, threads);
  p.grid = grid_for(threads, p.workgroup);
  if (quad) return p;
  /* streamed (non-temporal) PCM stores where the layout allows, from AAD_HIP_DECODE_NT_MIN lanes on (measurement aid, never
   * changes a byte) */
  p.stream_stores = b.stream_stores && b.channels == 2 && b.bits != 3 && lanes >= k.decode_nt_min;
  if (p.workgroup == 256u) p.lds = dense_decode_lds_pad(d, k, lanes, b.channels, b.bits);
  return p;
}

/* ---- window decode (AADHip_WindowDecodePlanRun): one lane per (window, block-in-window, channel) ---------------------------- */
struct WindowBatch {
  uint64_t windows;
  uint32_t frames, channels, bits, samples_per_block;
};
struct WindowLaunch {
  bool ok;                    /* false: N * C * T elements (or their bytes as float32) or the lane count overflow 64 bits */
  uint32_t blocks_per_window; /* K: the most blocks a window of `frames` frames can touch */
  uint32_t workgroup, grid, lds;
  uint64_t lanes;    /* windows * K * channels; the kernel walks them grid-stride when the grid is capped */
  uint64_t elements; /* windows * channels * frames */
};

/* blocks touched by frames [first, first + frames) when `first` sits `phase` frames into its block (frames >= 1) */
inline uint64_t window_blocks_at(uint64_t phase, uint64_t frames, uint64_t spb) { return (phase + frames - 1) / spb + 1; }
/* ... at the worst phase (spb - 1): ceil((frames - 1) / spb) + 1 */
inline uint64_t window_blocks_spanned(uint64_t frames, uint64_t spb) { return frames == 0 ? 0 : (frames - 1 + spb - 1) / spb + 1; }

/* 2^20 workgroups (2^28 threads at 256) and beyond that the kernel's grid-stride loop: a dispatch's grid is a 32-bit work-item count */
constexpr uint64_t kWindowMaxGrid = 1ull << 20;

/* The window kernel is the per-lane dense decoder with predicated stores: the dense decoder's workgroup rule (one-wave workgroups
 * while the batch has at most one wave per SIMD) and its occupancy cap (dense_decode_lds_pad) */
/* out_channels: the rows a window has in the output (`elements`), b.channels: the channels a window's lanes decode.  They differ
 * in a channel-mix run alone (plan_window_run). */
inline WindowLaunch plan_window_decode_into(const Device &d, const Knobs &k, const WindowBatch &b, uint32_t out_channels)
{
  WindowLaunch p = {};
  if (b.frames == 0 || b.samples_per_block == 0 || b.channels == 0 || out_channels == 0) return p;
  const uint64_t kb = window_blocks_spanned(b.frames, b.samples_per_block);
  uint64_t per_window = 0, elements = 0, bytes = 0;
  if (__builtin_mul_overflow(kb, (uint64_t)b.channels, &per_window) || __builtin_mul_overflow(b.windows, per_window, &p.lanes)) return p;
  if (__builtin_mul_overflow(b.windows, (uint64_t)out_channels * b.frames, &elements) || __builtin_mul_overflow(elements, (uint64_t)4, &bytes))
    return p;
  p.ok = true;
  p.blocks_per_window = (uint32_t)kb;
  p.elements = elements;
  if (p.lanes == 0) return p;
  p.workgroup = pick_workgroup(d, p.lanes);
  const uint64_t groups = (p.lanes + p.workgroup - 1) / p.workgroup;
  p.grid = (uint32_t)(groups < kWindowMaxGrid ? groups : kWindowMaxGrid);
  if (p.workgroup == 256u) p.lds = dense_decode_lds_pad(d, k, p.lanes, b.channels, b.bits);
  return p;
}
inline WindowLaunch plan_window_decode(const Device &d, const Knobs &k, const WindowBatch &b)
{
  return plan_window_decode_into(d, k, b, b.channels);
}

/* ---- window decode statistics (AADHip_WindowDecodePlanRunStats): the table of a run ------------------------------------------ */
struct WindowStatsTable {
  bool ok;        /* false: the pointer is null or not 8-byte aligned while the run has windows, or windows * channels * 32 bytes
                   * overflow 64 bits - with frames < 8 that can happen where the rows' bytes do not */
  uint64_t bytes; /* windows * out_channels * sizeof(AADHipRowStats): what the run clears in front of its first launch */
};
inline WindowStatsTable window_stats_table(uint64_t windows, uint32_t out_channels, uint64_t stats_address)
{
  WindowStatsTable t = {};
  uint64_t records = 0;
  if (__builtin_mul_overflow(windows, (uint64_t)out_channels, &records) ||
      __builtin_mul_overflow(records, (uint64_t)sizeof(struct AADHipRowStats), &t.bytes)) {
    t.bytes = 0;
    return t;
  }
  t.ok = windows == 0 || (stats_address != 0 && (stats_address & 7u) == 0);
  return t;
}

/* ---- mixed-format window decode (AADHip_MixedWindowDecodePlanCreate): one launch per kernel variant of the plan ------------- */
/* what a lane reads of its stream's format, one record per stream next to the descriptor table (device memory) */
struct StreamFormat {
  uint32_t samples_per_block;
  uint16_t block_size;
  uint8_t bits;
  uint8_t mid_side; /* 1: the M/S instantiation decodes this stream (two channels and the M/S method), else 0 */
};
static_assert(sizeof(StreamFormat) == 8, "per-stream format record");

/* mid/side is a kernel variant for two channels only: every other channel count runs the L/R instantiation whatever the method
 * says, as the launch nest does (the plan's validation refuses M/S there anyway) */
inline StreamFormat stream_format_of(const struct AADHeaderInfo &h, uint32_t channels)
{
  return StreamFormat{h.num_samples_per_block, h.block_size, (uint8_t)h.bits_per_sample,
                      (uint8_t)(channels == 2 && h.ch_process_method == AAD_CH_PROCESS_METHOD_MS)};
}

/* a kernel variant of a plan: the template parameters its streams need, and the smallest block among them (the launch's K).
 * channels: what a stream of the variant holds; 0 in a list stands for the plan's own count (a mixed plan's records do not hold
 * it), which plan_window_run puts in its place */
struct WindowVariant {
  uint32_t channels, bits, mid_side, min_samples_per_block, streams;
};
constexpr uint32_t kMaxWindowVariants = 9;
struct WindowVariants {
  uint32_t count;
  WindowVariant v[kMaxWindowVariants];
};

/* The builders below count every stream into its variant's slot - 4-bit L/R, 4-bit M/S, 3-bit L/R, 3-bit M/S, 2-bit L/R, 2-bit M/S,
 * then mono 4-, 3- and 2-bit (a channel-mix plan alone tells mono apart) - and list the slots that hold streams, in that order */
inline void count_window_stream(WindowVariant (&slot)[kMaxWindowVariants], bool mono_slot, uint32_t channels, uint32_t bits, bool mid_side,
                                uint32_t samples_per_block)
{
  WindowVariant &s = slot[mono_slot ? 6u + (4u - bits) : (4u - bits) * 2u + (mid_side ? 1u : 0u)];
  if (s.streams == 0 || samples_per_block < s.min_samples_per_block) s.min_samples_per_block = samples_per_block;
  s.channels = channels;
  s.bits = bits;
  s.mid_side = mid_side ? 1u : 0u;
  s.streams++;
}
inline WindowVariants window_variants_present(const WindowVariant (&slot)[kMaxWindowVariants])
{
  WindowVariants out = {};
  for (const WindowVariant &s : slot)
    if (s.streams != 0) out.v[out.count++] = s;
  return out;
}

/* The variants present in formats[0 .. n) of a mixed-format plan, each once, in the fixed order 4-bit L/R, 4-bit M/S, 3-bit L/R,
 * 3-bit M/S, 2-bit L/R, 2-bit M/S, every one of the plan's channel count.  Records with bits outside 2 .. 4 belong to no variant
 * (plan create has refused them). */
inline WindowVariants window_variants(const StreamFormat *formats, uint64_t n)
{
  WindowVariant slot[kMaxWindowVariants] = {};
  for (uint64_t i = 0; i < n; i++) {
    const StreamFormat &f = formats[i];
    if (f.bits < 2 || f.bits > 4) continue;
    count_window_stream(slot, false, 0, f.bits, f.mid_side != 0, f.samples_per_block);
  }
  return window_variants_present(slot);
}

/* ---- channel-mix window decode (AADHip_ChannelMixWindowDecodePlanCreate): mono and stereo streams into one channel count ---- */
/* which decoder a stream needs: the source channel count, and for two channels the inverse mid/side */
enum StreamSource : uint8_t { kSourceMono = 0, kSourceStereo = 1, kSourceMidSide = 2, kSourceNone = 3 };
/* StreamFormat with the source in the place of mid_side */
struct ChannelStreamFormat {
  uint32_t samples_per_block;
  uint16_t block_size;
  uint8_t bits;
  uint8_t source; /* a StreamSource; kSourceNone: a channel count other than 1 or 2 (plan create has refused it) */
};
static_assert(sizeof(ChannelStreamFormat) == 8, "per-stream format record");

/* a mono stream is kSourceMono whatever its method says (the plan's validation refuses M/S there anyway) */
inline ChannelStreamFormat channel_stream_format_of(const struct AADHeaderInfo &h)
{
  const uint8_t source = h.num_channels == 1   ? kSourceMono
                         : h.num_channels != 2 ? kSourceNone
                         : h.ch_process_method == AAD_CH_PROCESS_METHOD_MS ? kSourceMidSide
                                                                           : kSourceStereo;
  return ChannelStreamFormat{h.num_samples_per_block, h.block_size, (uint8_t)h.bits_per_sample, source};
}

/* The variants present in formats[0 .. n) of a channel-mix plan, each once: window_variants' six stereo ones in its order, then
 * mono 4-, 3- and 2-bit.  Records with bits outside 2 .. 4 or without a source belong to no variant. */
inline WindowVariants channel_mix_variants(const ChannelStreamFormat *formats, uint64_t n)
{
  WindowVariant slot[kMaxWindowVariants] = {};
  for (uint64_t i = 0; i < n; i++) {
    const ChannelStreamFormat &f = formats[i];
    if (f.bits < 2 || f.bits > 4 || f.source >= kSourceNone) continue;
    const bool mono = f.source == kSourceMono;
    count_window_stream(slot, mono, mono ? 1u : 2u, f.bits, f.source == kSourceMidSide, f.samples_per_block);
  }
  return window_variants_present(slot);
}

/* ---- the launches of a window decode run, whatever the plan's kind ---------------------------------------------------------- */
/* Same: AADHip_WindowDecodePlanCreate, one format - its list is the one variant of that header; Mixed, ChannelMix: above */
enum class WindowKind : uint32_t { Same = 0, Mixed = 1, ChannelMix = 2 };

struct WindowRunPlan {
  bool ok;        /* false: some launch's lane count, or the output's elements or bytes, overflow 64 bits - nothing is launched */
  uint32_t count; /* launches of the run: one per variant, and ONE for a plan without variants (num_streams == 0) */
  WindowVariant variant[kMaxWindowVariants];
  WindowLaunch launch[kMaxWindowVariants]; /* launch[0] also writes the zeros of the windows whose stream is out of range */
};

/* Every launch walks all the windows and is planned by plan_window_decode_into's rules with its variant's bits and smallest block:
 * K covers that variant's every stream, the lanes past a stream's own last covering block leave.  A launch's lanes are (window,
 * block, SOURCE channel) of its variant, and `elements` is the output's, windows * out_channels * frames, whose overflow refuses
 * the run whatever the sources; the two channel counts differ in a channel-mix run alone, which has one or two rows per window.
 * A plan without variants has no stream a window could name: its one launch over blocks of `frames` frames only writes zeros - the
 * 4-bit L/R kernel of out_channels channels, and in a channel-mix run the mono 4-bit kernel (one lane per window and block covers
 * out_channels rows). */
inline WindowRunPlan plan_window_run(const Device &d, const Knobs &k, WindowKind kind, const WindowVariants &variants, uint64_t windows,
                                     uint32_t frames, uint32_t out_channels)
{
  WindowRunPlan m = {};
  const bool mix = kind == WindowKind::ChannelMix;
  WindowVariants vs = variants;
  if (vs.count == 0) vs.v[vs.count++] = WindowVariant{mix ? 1u : out_channels, 4, 0, frames, 0};
  if (vs.count > kMaxWindowVariants || (mix && (out_channels < 1 || out_channels > 2))) return m;
  for (uint32_t i = 0; i < vs.count; i++) {
    WindowVariant &v = m.variant[i] = vs.v[i];
    if (v.channels == 0) v.channels = out_channels;
    m.launch[i] = plan_window_decode_into(d, k, WindowBatch{windows, frames, v.channels, v.bits, v.min_samples_per_block}, out_channels);
    if (!m.launch[i].ok) return m;
  }
  m.count = vs.count;
  m.ok = true;
  return m;
}

/* plan_window_run under the names of the two kinds that plan more than one launch, as tests/mixed_window_policy_driver.cpp and
 * tests/channel_mix_policy_driver.cpp call it */
using MixedWindowLaunch = WindowRunPlan;
using ChannelMixVariants = WindowVariants;
using ChannelMixWindowLaunch = WindowRunPlan;
inline WindowRunPlan plan_mixed_window_decode(const Device &d, const Knobs &k, const WindowVariants &variants, uint64_t windows,
                                              uint32_t frames, uint32_t channels)
{
  return plan_window_run(d, k, WindowKind::Mixed, variants, windows, frames, channels);
}
inline WindowRunPlan plan_channel_mix_window_decode(const Device &d, const Knobs &k, const WindowVariants &variants, uint64_t windows,
                                                    uint32_t frames, uint32_t out_channels)
{
  return plan_window_run(d, k, WindowKind::ChannelMix, variants, windows, frames, out_channels);
}

} /* namespace aad */

#endif /* AAD_LAUNCH_POLICY_H */
