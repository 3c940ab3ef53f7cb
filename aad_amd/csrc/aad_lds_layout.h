/* aad_lds_layout.h - the kernels' LDS layouts as plain constants, read by the kernels and by the host compiler: the launch policy
 * (aad_launch_policy.h) takes its residency and dynamic-LDS decisions from the same numbers the kernels are built with. */
#ifndef AAD_LDS_LAYOUT_H
#define AAD_LDS_LAYOUT_H

#include <stdint.h>

#include "aad_tables_data.h"

namespace aad {
constexpr int kTaps = 4;
constexpr int kBlockHeaderBytesPerCh = 18;
constexpr int kFileHeaderBytes = 31;
constexpr int kChunk = 16; /* samples per unrolled chunk: a multiple of every pack unit (2, 8, 4) and of the tap count */

/*
 * LDS image (one per workgroup, ~3.3 KB).  Dense dword arrays so that a lookup is bank-conflict
 * free unless two lanes hit different entries 32 apart:
 *   step[256]   uint32   step size
 *   hr[256]     float    fl32(0.5 / step)
 *   hs[256]     float    2^(BITS-1) * hr
 *   code[16]    {int32 sm21, int16 delta | bias << 16}   decoder: everything a code implies, 8 bytes -
 *               sixteen records fill exactly one row of the 32 LDS banks, so a ds_read_b64 in which
 *               every lane asks for a different code is conflict-free (the 16-byte {sm21, bias,
 *               delta, -} records of round 1 put codes c and c + 8 - same magnitude, other sign - on
 *               the same banks: 3.8 conflict cycles per lookup in the dense decoder)
 *   delta[8]    int16    encoder: index delta by magnitude
 * (A first layout used one 16-byte record per step: only 8 bank groups, SQ_LDS_BANK_CONFLICT was
 * half of all LDS cycles and lookups on the recurrence's critical path took ~100 cycles.)
 * The Q4 step index is kept biased by +8 (idxb), so its table slot is idxb >> 4.
 */
constexpr int kIdxBias = 8;
constexpr int kIdxMin = kIdxBias, kIdxMax = AAD_STEP_INDEX_MAX + kIdxBias;
/* Largest step index a BLOCK HEADER may carry and still mean something in the reference: the 12-bit field is taken as it is
 * (src/aad_decoder.c:365-366, no clamp), the first sample's step is T[(idx + 8) >> 4] (src/aad_tables.h:15,28) - slot 255 for
 * 4081..4087 as for 4080 - and the index walk goes on from the UNCLAMPED value (clamp(idx + delta, 0, 4080), :31-43), so a
 * header index of 4087 followed by a delta of -18 gives 4069, not 4062.  4088..4095 make the reference read past its
 * 256-entry table (undefined there); they are taken as 4087 here. */
constexpr int kHeaderIdxMax = AAD_STEP_INDEX_MAX + 7;
constexpr int kLdsStepOff = 0, kLdsHrOff = 1024, kLdsHsOff = 2048;
constexpr int kLdsCodeOff = 3072;
constexpr int kLdsCodeShift = 3; /* log2 of the record size */
constexpr int kLdsDeltaOff = kLdsCodeOff + (16 << kLdsCodeShift);
constexpr int kLdsDeltaScaledOff = kLdsDeltaOff + 16; /* the same eight deltas times kIdxScale (encoders' scaled step index) */
constexpr int kLdsBytes = kLdsDeltaScaledOff + 16;
/* Quad kernels only: the same three values as 16-byte records {step, hr, hs, -}, addressed by
 * idxb & 0xFF0 - one instruction less than slot_addr and one lookup instead of two.  A wave of
 * the quad mapping holds just 16 distinct recurrences, so the 8-bank-group stride that made this
 * layout an 8-way conflict with 64 recurrences per wave is harmless here. */
constexpr int kLdsWideOff = (kLdsBytes + 15) & ~15;
constexpr int kLdsBytesQuad = kLdsWideOff + AAD_STEP_TABLE_LEN * 16;
/* ENCODERS: kWideCopies copies of the wide records, interleaved - slot i, copy k at 16 (kWideCopies i + k).
 * A ds_read_b96 is served eight lanes per LDS cycle, and the eight are NOT neighbours: the groups are
 * {0-3, 20-23}, {4-7, 16-19}, {8-11, 28-31}, {12-15, 24-27} and the same in the upper half of the wave
 * (MI355X_MICROARCH.md, LDS table), over 32 banks.  A group is therefore four lanes of an even 16-lane row
 * and four of an odd one - in the tap-major quad layout two taps of EIGHT different recurrences, in the
 * dense mapping eight recurrences outright - and every one of the eight may ask for another slot.  Round 2
 * kept four copies (copy = lane & 3) at a 64-byte pitch on the belief that a group was eight adjacent
 * lanes: the two lanes that share a copy collide whenever their slots agree mod 2 - SQ_LDS_BANK_CONFLICT
 * 7.1 cycles per lookup in the headline kernel (profiles/r02_pmc_summary_bench.txt), on the one lookup
 * that sits on the recurrence.  With eight copies at a 128-byte pitch, copy = (lane & 3) | row parity << 2,
 * the lanes of a group own banks 4 copy .. 4 copy + 2 whatever their slots: no two reads of a cycle meet.
 * The encoders keep the step index scaled by kIdxScale = kWideCopies for this (J = kIdxScale * idxb; the
 * slot is J >> 7 and the address (J & 0x7F80) | 16 copy: one v_and_or_b32, where the unscaled form took one
 * v_and_b32); the index deltas come scaled as well.  AAD_WIDE_COPIES=4 rebuilds round 2's layout (A/B). */
#ifndef AAD_WIDE_COPIES
#define AAD_WIDE_COPIES 8
#endif
constexpr int kWideCopies = AAD_WIDE_COPIES;
static_assert(kWideCopies == 4 || kWideCopies == 8, "four (round 2) or eight copies of the encoders' step records");
constexpr int kIdxScale = kWideCopies;
constexpr int kIdxScaleLog2 = kWideCopies == 8 ? 3 : 2;
constexpr int kLdsBytesQuadEnc = kLdsWideOff + AAD_STEP_TABLE_LEN * 16 * kWideCopies;
/* Dense DECODER: step << 2 in four copies per 16-byte slot (copy = lane & 3 spreads a wave's lookups
 * over all banks; the slot's address is idxb & 0xFF0, one v_and_or_b32 with the copy offset) and
 * 16-byte per-code records {bias << 29 | delta & 0xFFFF, 0, sm21 << 27, -} for the one-instruction
 * dequantiser (dense_dequantise). */
constexpr int kLdsDenseStepOff = (kLdsBytes + 15) & ~15;
constexpr int kLdsDenseCodeOff = kLdsDenseStepOff + AAD_STEP_TABLE_LEN * 16;
/* the same records in 8 bytes {bias << 29 | delta & 0xFFFF, sm21 << 27} (the addend's upper word is zero and costs the
 * reader one v_mov_b32): sixteen of them are one row of the 64 banks a ds_read_b64 sees - no two codes share a bank,
 * where the 16-byte records put codes c and c + 8 on the same banks and every ds_read_b96 takes eight LDS cycles.
 * For the kernels whose waves share a busy LDS (the sector-tiled dense decoder) - a lone wave prefers the one wide
 * lookup without the v_mov. */
constexpr int kLdsDenseCode8Off = kLdsDenseCodeOff + 16 * 16;
constexpr int kLdsBytesDenseDec = kLdsDenseCode8Off + 16 * 8;

/* which dense encoders stage their codes, where the staging area starts in their LDS block, and its size */
template <int BITS, int CHF, bool QUAD>
constexpr bool kStagedCodes = !QUAD && (CHF == 1 || (CHF == 2 && BITS != 4));
constexpr int kLdsCodeStageOff = (kLdsBytesQuadEnc + 15) & ~15;
template <int BITS, int CHF, bool QUAD>
constexpr int kLdsBytesEncoder = kStagedCodes<BITS, CHF, QUAD> ? kLdsCodeStageOff + 4 * 8 * 64 * (BITS == 2 ? 4 : 8) : kLdsBytesQuadEnc;
/* the instantiations that move their output through ByteRing: dense, mono / stereo, 4- and 2-bit codes (pieces of whole dwords) */
template <int BITS, int CHF, bool QUAD>
constexpr bool kRingable = !QUAD && (CHF == 1 || CHF == 2);
/* The rows' byte rings live in DYNAMIC LDS, one wave's worth per wave of the workgroup (the launch asks for blockDim.x / 64 of
 * them): a static area for four waves cost the one-wave workgroups of 16 385 .. 65 536-lane batches a resident wave per CU
 * (72 864 B mono / 54 432 B stereo 4-bit per workgroup instead of 45 216 / 40 608). */
template <int CHF>
constexpr int kLdsRingBytesPerWave = (64 / (CHF ? CHF : 1)) * 144;
template <int BITS, int CHF, bool QUAD, bool RING>
constexpr int kLdsBytesEncoderStatic = RING ? kLdsCodeStageOff : kLdsBytesEncoder<BITS, CHF, QUAD>;

/* LDS-resident residuals: rows of kLdsResidualRow dwords, enough for blocks of up to
 * kLdsResidualMax coded samples per channel (every 4-bit geometry up to max_block_size 1024 and
 * most others); the row length is 20 mod 32 dwords so that the sixteen rows a wave reads at the
 * same sample offset spread over the banks.  132 KB of the CU's 160 KB: one workgroup per CU,
 * which is what this path is for (the host uses it up to one workgroup per CU). */
constexpr uint32_t kLdsResidualMax = 2048;
constexpr uint32_t kLdsResidualRow = kLdsResidualMax + kChunk + 4;
constexpr int kTiledWaves = 4; /* waves per workgroup of the sector-tiled dense decoder (aad_decode_tiled.hip.h DecodeTile) */

} /* namespace aad */

#endif /* AAD_LDS_LAYOUT_H */
