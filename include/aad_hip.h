/*
 * aad_hip.h - additive batched C-ABI of the MI355X AAD engine (SURVEY.md section 8b "New (additive) ABI").
 *
 * The reference has no batched or device-resident entry point: its only data path is one stream
 * per call through AADEncoder_EncodeWhole (src/aad_encoder.c:814-891), AADDecoder_DecodeWhole
 * (src/aad_decoder.c:478-538) and AADDecoder_DecodeBlock (src/aad_decoder.c:321-475).  A GPU is
 * only useful when many independent units are in flight (encode: stream x channel; decode:
 * block x channel), so this header exposes exactly those three loops over MANY streams:
 *
 *   AADHip_EncodePlanRun  == for each stream: the block loop of AADEncoder_EncodeWhole
 *                            (EncodeHeader + [SearchBestProcessor] + EncodeBlock per block)
 *   AADHip_DecodePlanRun  == for each stream: the block loop of AADDecoder_DecodeWhole
 *                            (DecodeBlock per block), every block decoded independently
 *
 * Plain C: pointers and sizes only.  "Device" pointers are HIP device addresses (hipMalloc or
 * any allocator sharing the HIP context, e.g. a torch tensor's data_ptr()).  The legacy
 * AADEncoder_ / AADDecoder_ symbols are implemented on top of these with a batch of one.
 *
 * Device data layout
 *   PCM   : int16, channel-interleaved frames, one contiguous run per stream (AADHip_PlanarEncodePlanRun: int16 or
 *           float32 rows, one per channel).
 *   .aad  : the exact file image per stream - 31-byte header followed by the blocks - byte for
 *           byte what the reference writes for the same samples and parameters.
 */
#ifndef AAD_HIP_H_INCLUDED
#define AAD_HIP_H_INCLUDED

#include <stdint.h>
#include "aad.h"
#include "aad_encoder.h"

#define AAD_HIP_MAX_NUM_CHANNELS 8 /* container extension; the legacy API keeps AAD_MAX_NUM_CHANNELS */

struct AADHipContext;    /* device + stream + device-side tables */
struct AADHipEncodePlan; /* uploaded stream table + launch geometry for one parameter set */
struct AADHipDecodePlan;

/* One stream of a batch.  Offsets are relative to the buffers handed to ...PlanRun. */
struct AADHipStreamDesc {
  uint64_t pcm_offset;  /* index of the stream's first int16 in the PCM buffer */
  uint64_t data_offset; /* byte offset of the stream's .aad image in the data buffer */
  uint64_t data_size;   /* encode: capacity in bytes; decode: bytes present (a short last block is fine) */
  uint32_t num_samples; /* samples per channel */
  uint32_t reserved;
};

/* Predictor state of one stream x channel, carried across calls exactly like the reference's
 * struct AADEncodeProcessor (src/aad_encoder.c:10-15) inside a reused encoder handle.
 *
 * What a run does with a record it is handed (every entry point that takes state; tests/test_gpu_crafted_state.py):
 *   - stepsize_index is clamped to [0, 4080] on load: a run given an index outside that range computes exactly what it computes
 *     given the clamped index.  (The reference keeps the index in an int16 and asserts the range.)
 *   - weight[] is taken as it is, any int32.  The first block header carries weight >> shift with the smallest shift that brings
 *     the largest magnitude to 16 bits and the shifted-out bits cleared in the carried weights too; the header's 4-bit field holds
 *     shift & 15, so magnitudes from 2^30 on (shift 16) wrap it, as in the reference built with NDEBUG.  INT32_MIN, whose
 *     magnitude does not exist in int32, never becomes the largest magnitude: next to smaller weights its header field reads 0.
 *   - history[] is overwritten at every block start with the block's first four samples (taps that no sample seeds: 0), so its
 *     contents before a run do not matter.
 *   - quantize_error is the dequantised difference of the last coded sample.  The first four samples of a block travel in its
 *     header and are not coded: a run that codes no sample of a stream (1 .. 4 samples) passes quantize_error through untouched.
 * The record written back holds the weights, history and index the next block would start from. */
struct AADHipLaneState {
  int32_t weight[4];
  int32_t history[4];
  int32_t stepsize_index;
  int32_t quantize_error;
};

#ifdef __cplusplus
extern "C" {
#endif

/* number of usable HIP devices (0 when there is none; never fails) */
int32_t AADHip_GetDeviceCount(void);

/* Create a context on `device_index`.  `hip_stream` is a hipStream_t the caller owns, or NULL
 * to let the context create (and later destroy) its own stream.  All ...Run calls are
 * asynchronous on that stream. */
AADApiResult AADHip_ContextCreate(int32_t device_index, void *hip_stream, struct AADHipContext **context);
void AADHip_ContextDestroy(struct AADHipContext *context);
AADApiResult AADHip_ContextSynchronize(struct AADHipContext *context);
/* text of the last HIP failure seen by this context ("" if none); valid until the next call */
const char *AADHip_ContextLastError(const struct AADHipContext *context);

/* Cross-stream ordering and kernel timing without packets of their own.  `hip_start_event` / `hip_stop_event` (hipEvent_t the
 * caller owns; either may be NULL, both NULL withdraws) are recorded when the work of the NEXT AADHip_EncodePlanRun /
 * AADHip_PlanarEncodePlanRun / AADHip_PlanarReconstructPlanRun / AADHip_PlanarReconstructPlanRunStats / AADHip_WindowReconstructPlanRun / AADHip_DecodePlanRun / AADHip_WindowDecodePlanRun / AADHip_WindowDecodePlanRunStats / AADHip_WindowDecodePlanRunGain / AADHip_WindowDecodePlanRunPlaced / AADHip_WindowDecodePlanRunPlacedStats / AADHip_ReconstructPlanRun call on this context starts / is done - one-shot:
 * the run takes them.  An encode, decode or window decode plan run is one kernel (a mixed-format or channel-mix window decode several: start on the first, stop on
 * the last; a run that first clears a statistics table - AADHip_WindowDecodePlanRunStats, a segmented AADHip_PlanarReconstructPlanRunStats - records the
 * start event with hipEventRecord in front of the clear and its last kernel carries the stop event), and the events ride on that kernel's own dispatch (hipExtLaunchKernelGGL's start and
 * stop events) instead of on barrier packets around it: a hipEventRecord behind every launch of a back-to-back sequence costs
 * the queue 2.9 us per launch on MI355X, the attached event nothing (profiles/r03_microbench_event_gap.txt), and
 * hipEventElapsedTime between the two is the kernel's own duration.  Another stream waits for the stop event with
 * hipStreamWaitEvent as usual.  A run that fails leaves the events unrecorded; the host-memory calls (...Batch, the legacy API)
 * do not look at them. */
AADApiResult AADHip_ContextSignalNextRun(struct AADHipContext *context, void *hip_start_event, void *hip_stop_event);
/* NOT available when the process runs with ROC_SYSTEM_SCOPE_SIGNAL=0 (a ROCm runtime setting that gives kernel dispatches
 * device-scope completion signals): the stop event IS the kernel's completion signal, and another stream's
 * hipStreamWaitEvent on it would never return.  A context created under that setting refuses the call - AAD_APIRESULT_NG,
 * AADHip_ContextLastError says why - instead of letting the caller hang; withdrawing (both NULL) always succeeds, and
 * hipEventRecord behind the run remains the portable way.  AADHip_SignalNextRunSupported: 1, or 0 under that setting
 * (reads the environment, needs no device). */
int32_t AADHip_SignalNextRunSupported(void);

/* Launch options of a context.  Defaults: the environment variables AAD_HIP_MAPPING
 * (auto | dense | quad | quad-fused | dense-tiled), AAD_HIP_TRIAL_LANES (dual | single),
 * AAD_HIP_STAGING_THREADS (1..8) and AAD_HIP_TILE_KBYTES, read ONCE when the context is created; the library does not read them
 * again (the measurement aids of INTEGRATION.md section 4 - AAD_HIP_ENCODE_RING, ..._LDS_PAD - are not options and never change a byte).  An option holds for every later
 * ...Run / ...Batch call of the context; set it from the thread that owns the context. */
enum AADHipOption {
  AAD_HIP_OPTION_LANE_MAPPING = 0, /* enum AADHipLaneMapping */
  AAD_HIP_OPTION_TRIAL_LANES = 1,  /* enum AADHipTrialLanes */
  /* Threads that copy between the caller's buffers and the pinned staging blocks in the host-memory
   * entry points (...Batch, EncodeWhole/DecodeWhole), the caller's own included: 0 = by core count
   * (8 from thirty-two cores, 4 from eight, 2 from four), 1 = the caller alone (no helper thread is ever started),
   * up to 8.  Helpers start at the first chunk of a megabyte or more and end in ContextDestroy. */
  AAD_HIP_OPTION_STAGING_THREADS = 2,
  /* Budget, in KiB, of one tile of the host-memory entry points (input + output bytes that travel
   * together; see DESIGN.md "host-memory path"): 0 = built in (batches up to 16 MiB go as one tile,
   * larger ones in tiles of about 16 MiB).  A tile never holds less than one block of one stream.  Default from
   * AAD_HIP_TILE_KBYTES.  Results do not depend on it. */
  AAD_HIP_OPTION_TILE_KBYTES = 3,
  /* Order of the fp64 sums behind the reconstruction modes' RMSE / MSD (AADHip_Reconstruct*): 0 = a fixed tree on the
   * device, with the reference's channel-major sequential order taken per stream only when the tree's result lies so close
   * to a rounding boundary of the six decimals `aad -c` prints that the order could show (the printed line is the
   * reference's either way); 1 = always the reference's order (bit-identical doubles, one lane per stream: slow).
   * Default from AAD_HIP_COMPARE_ORDER (auto | sequential). */
  AAD_HIP_OPTION_COMPARE_ORDER = 4,
  /* enum AADHipSimdRole: the SIMD of a compute unit that runs the one busy wave per workgroup of this context's lane-starved
   * launches (the quad encoder of up to 16 recurrences per compute unit of the device, the split decoder's recurrence wave).
   * Contexts whose kernels run side by side on one device - the engines of step pipelines - take different SIMDs, so that no two
   * of those waves share one.  Off (the default): the launches as they are without the option.  The bytes never depend on it. */
  AAD_HIP_OPTION_SIMD_ROLE = 5
};
enum AADHipSimdRole {
  AAD_HIP_SIMD_ROLE_OFF = -1,
  AAD_HIP_SIMD_ROLE_0 = 0, AAD_HIP_SIMD_ROLE_1 = 1, AAD_HIP_SIMD_ROLE_2 = 2, AAD_HIP_SIMD_ROLE_3 = 3
};
enum AADHipLaneMapping {
  AAD_HIP_LANE_MAPPING_AUTO = 0,      /* by batch size (the default) */
  AAD_HIP_LANE_MAPPING_DENSE = 1,     /* one lane per recurrence */
  AAD_HIP_LANE_MAPPING_QUAD = 2,      /* four lanes per recurrence; decode: step-index scan on other waves */
  AAD_HIP_LANE_MAPPING_QUAD_FUSED = 3, /* four lanes per recurrence; decode: one fused kernel */
  AAD_HIP_LANE_MAPPING_DENSE_TILED = 4 /* one lane per recurrence, memory moved in whole sectors / lines through LDS where the layout allows (else: dense) */
};
enum AADHipTrialLanes {
  AAD_HIP_TRIAL_LANES_DUAL = 0,  /* trial search on the quad mapping: a second group of lanes runs the probe and encodes every candidate beside the chain
                                  * (batches of up to 5120 recurrences, where it pays; larger ones take the other layout) */
  AAD_HIP_TRIAL_LANES_SINGLE = 1 /* both strands on the same lanes */
};
AADApiResult AADHip_ContextSetOption(struct AADHipContext *context, int32_t option, int32_t value);

/* bytes of the .aad image of a stream (header + full blocks + short tail); 0 on a bad parameter.
 * Same arithmetic as the write_offset AADEncoder_EncodeWhole ends with (src/aad_encoder.c:881-889). */
uint64_t AADHip_CalculateEncodedSize(const struct AADEncodeParameter *parameter, uint32_t num_samples);

/* ---- encode ------------------------------------------------------------------------------ */

/* Validates `parameter` like AADEncoder_SetEncodeParameter + AADEncoder_EncodeHeader would
 * (INVALID_FORMAT), checks every stream's capacity (INSUFFICIENT_BUFFER) and uploads the table.
 * `streams` is a host array. */
AADApiResult AADHip_EncodePlanCreate(
    struct AADHipContext *context, const struct AADEncodeParameter *parameter,
    uint32_t num_streams, const struct AADHipStreamDesc *streams,
    struct AADHipEncodePlan **plan);
void AADHip_EncodePlanDestroy(struct AADHipEncodePlan *plan);

/* Encode every stream of the plan.  device_state: NULL for fresh encoders (zero weights, zero
 * step index), else num_streams * num_channels records read before and written after the run. */
AADApiResult AADHip_EncodePlanRun(
    struct AADHipEncodePlan *plan, const int16_t *device_pcm, uint8_t *device_data,
    struct AADHipLaneState *device_state);

/* ---- segmented encode: long streams as parallel block chains -------------------------------- */

/* An encode plan is one serial chain of blocks per stream and channel: the weights and the step index carry from each block to
 * the next (src/aad_encoder.c:853-886), so a run takes as long as the longest stream's block count, however many streams share
 * it.  Every block header carries the decoder's whole state (src/aad_decoder.c:362-379) and decoding never looks across a block
 * boundary, so a segmented plan cuts each stream into segments encoded by independent chains side by side.
 *
 * Definition.  A stream of N frames has B = ceil(N / spb) blocks (spb: samples per block of the parameter's geometry).  With
 * L = segment_blocks and W = warmup_blocks, segment s keeps blocks [s L, min((s + 1) L, B)); with w = min(W, s L) its bytes are
 * those of a fresh reference encoder (AADEncoder_Create, AADEncoder_SetEncodeParameter with the same parameter and trial
 * count, AADEncoder_EncodeWhole) over frames [(s L - w) spb, min((s + 1) L spb, N)), without its file header and without its
 * first w blocks (the warm-up).  The image is the stream's 31-byte file header with the whole stream's N, then the segments'
 * bytes in order: AADHip_CalculateEncodedSize bytes, as for any plan.  The bytes depend on the PCM, the parameter, L and W only.
 *
 * The image is a valid format-v4 stream that any decoder (the reference's included) decodes to what the chains reconstructed.
 * It is NOT the reference encoder's bytes unless L >= B (or W >= (segments - 1) L): each chain starts from a fresh state, and the
 * warm-up does not converge onto the serial encode's.  The quality cost, the RMSE of the decoded image against the serial
 * encode's, depends on the signal, L and W; tools/segment_quality.py measures it ("Segmented encode").
 *
 * AADHip_SegmentedEncodePlanCreate validates `parameter` and `streams` exactly like AADHip_EncodePlanCreate (same errors) and
 * returns an ordinary plan: AADHip_EncodePlanRun, AADHip_EncodePlanDestroy and AADHip_ContextSignalNextRun work on it.
 * AAD_APIRESULT_INVALID_ARGUMENT: a null `segmentation`, segment_blocks == 0, more than UINT32_MAX segments in the batch, and
 * from AADHip_EncodePlanRun a non-null device_state (a segmented plan always starts from fresh encoders and leaves no state). */
struct AADHipSegmentation {
  uint32_t segment_blocks; /* L >= 1: blocks kept per chain */
  uint32_t warmup_blocks;  /* W: blocks encoded before a segment and discarded (clamped at the stream's start) */
};
AADApiResult AADHip_SegmentedEncodePlanCreate(
    struct AADHipContext *context, const struct AADEncodeParameter *parameter,
    const struct AADHipSegmentation *segmentation,
    uint32_t num_streams, const struct AADHipStreamDesc *streams,
    struct AADHipEncodePlan **plan);

/* ---- decode ------------------------------------------------------------------------------ */

/* `format` supplies channels / bits / block geometry / channel process method for the whole
 * batch (its num_samples field is ignored; each stream's count comes from `streams`).
 * Validated like AADDecoder_SetHeader (src/aad_decoder.c:173-225) with the channel limit raised
 * to AAD_HIP_MAX_NUM_CHANNELS.  has_file_header: non-zero when each image starts with the
 * 31-byte file header (DecodeWhole), zero when data_offset points at a bare block (DecodeBlock). */
AADApiResult AADHip_DecodePlanCreate(
    struct AADHipContext *context, const struct AADHeaderInfo *format, int32_t has_file_header,
    uint32_t num_streams, const struct AADHipStreamDesc *streams,
    struct AADHipDecodePlan **plan);
void AADHip_DecodePlanDestroy(struct AADHipDecodePlan *plan);

AADApiResult AADHip_DecodePlanRun(
    struct AADHipDecodePlan *plan, const uint8_t *device_data, int16_t *device_pcm);

/* ---- window decode: sample-accurate crops into planar int16 / float32 rows ------------------ */

/* Every block header carries the decoder's whole state (src/aad_decoder.c:362-379), so any stretch of a stream decodes from the
 * blocks that cover it alone.  A window decode plan holds a stream table; each run takes a table of windows FROM DEVICE MEMORY
 * (the host never reads it: windows drawn on the device, e.g. by torch.randint, need no synchronisation) and writes every window
 * as planar rows.
 *
 * Definition.  Let D_s be what AADHip_DecodePlanRun writes for stream s of the same format, has_file_header and table into a
 * zero-filled buffer of num_samples frames.  Then for window w = {stream, first_frame}, channel c < C and t < T:
 *   out[(w * C + c) * T + t] = D_s[first_frame + t][c]   converted to the sample type,
 * 0 where first_frame + t >= num_samples, and the whole window is 0 where stream >= num_streams.  Huge or "negative" (wrapped
 * int64) values are not an error: they give zeros and read nothing.  As under AADHip_DecodePlanRun no byte outside
 * [data_offset, data_offset + data_size) of a stream is read, and a truncated image decodes the same.
 *
 * AADHip_WindowDecodePlanCreate validates `format`, the flag and the table exactly as AADHip_DecodePlanCreate does (same errors);
 * pcm_offset is ignored.  One plan serves any number of windows and any window length.
 * AADHip_WindowDecodePlanRun: one kernel (AADHip_ContextSignalNextRun's events ride on it), asynchronous on the context's stream.
 * device_windows: num_windows records, 8-byte aligned (a contiguous torch int64 tensor [N, 2] on the device IS the table);
 * device_out: N * C * T samples.  num_windows == 0 is OK and launches nothing.  AAD_APIRESULT_INVALID_ARGUMENT for
 * frames_per_window == 0, an unknown sample_type, a null pointer while num_windows > 0, and N * C * T elements (or their float32
 * bytes) or the kernel's lane count N * (ceil((T - 1) / spb) + 1) * C overflowing 64 bits. */
struct AADHipWindow {
  uint64_t stream;      /* index into the plan's stream table */
  uint64_t first_frame; /* first frame of the window */
};
/* AAD_HIP_SAMPLE_FLOAT16 and AAD_HIP_SAMPLE_BFLOAT16: 2-byte float rows for a model under autocast, without a cast pass over a
 * float32 batch.  They are sample types of AADHip_WindowDecodePlanRun, AADHip_WindowDecodePlanRunStats, AADHip_WindowDecodePlanRunGain and AADHip_WindowDecodePlanRunPlaced alone, for plans of all
 * three constructors; the planar encode, planar reconstruct and window reconstruct entry points refuse them, and 2 and 3 are no
 * sample type anywhere.
 *
 * Definition.  Let f be the float32 value an AAD_HIP_SAMPLE_FLOAT32 run writes to the element: the int16 sample * 2^-15, and for
 * the stereo-to-mono down-mix of a channel-mix plan (L + R) * 2^-16 - both exact in float32.  FLOAT16 writes f rounded to IEEE
 * binary16, round to nearest even, subnormals kept; BFLOAT16 writes f rounded to bfloat16, round to nearest even.  One rounding,
 * taken from f: bit for bit torch's row_float32.to(torch.float16) and .to(torch.bfloat16).  Zeros are +0 (frames past num_samples,
 * stray windows, wrapped values).  Consequences, checked over all 65 536 int16 values:
 *   - sample 1 is binary16 0x0200, a subnormal, and -1 is 0x8200; no non-zero value rounds to zero, the smallest down-mix sum
 *     (2^-16, binary16 0x0100) included;
 *   - 32767 rounds to +1.0 in both types; -32768 and -32767 both give -1.0 in float16;
 *   - float16 is exact for 12 288 of the 65 536 values (|sample| <= 2048, then the multiples of 2, 4, 8, 16), bfloat16 for 2 304;
 *   - float16 has a tie at every odd |sample| in [2048, 4096): 2049 goes to 2048 and 2051 to 2052; bfloat16 has one at every
 *     odd |sample| in [256, 512): 257 goes to 256 and 259 to 260.
 * The statistics of AADHip_WindowDecodePlanRunStats are those of the int16 values, whatever the sample type.  Errors, the
 * alignment of device_out and the 64-bit size rule are those of int16: 2-byte elements. */
enum AADHipSampleType {
  AAD_HIP_SAMPLE_INT16 = 0,   /* the decoded sample */
  AAD_HIP_SAMPLE_FLOAT32 = 1, /* the decoded sample / 32768.0f (exact) */
  AAD_HIP_SAMPLE_FLOAT16 = 4, /* window decode only: the float32 value rounded to binary16, nearest even */
  AAD_HIP_SAMPLE_BFLOAT16 = 5 /* window decode only: the float32 value rounded to bfloat16, nearest even */
};
struct AADHipWindowDecodePlan;
AADApiResult AADHip_WindowDecodePlanCreate(
    struct AADHipContext *context, const struct AADHeaderInfo *format, int32_t has_file_header,
    uint32_t num_streams, const struct AADHipStreamDesc *streams,
    struct AADHipWindowDecodePlan **plan);
void AADHip_WindowDecodePlanDestroy(struct AADHipWindowDecodePlan *plan);
AADApiResult AADHip_WindowDecodePlanRun(
    struct AADHipWindowDecodePlan *plan, const uint8_t *device_data,
    uint64_t num_windows, const struct AADHipWindow *device_windows,
    uint32_t frames_per_window, int32_t sample_type, void *device_out);

/* Window decode over a corpus whose streams do not share a format: files encoded at different times, or streams encoded with the
 * bits AADHip's error statistics say each one needs.  A constructor of its own that returns an ordinary window decode plan:
 * AADHip_WindowDecodePlanRun, AADHip_WindowDecodePlanDestroy and AADHip_ContextSignalNextRun work on it unchanged.
 *
 * Definition.  The one above with one change: D_s is what AADHip_DecodePlanRun writes for stream s under formats[s] (with the
 * plan's has_file_header and the descriptor's data_offset, data_size and num_samples).  Samples past num_samples are zero, a
 * window with stream >= num_streams is all zero, wrapped int64 values give zeros and read nothing, no byte outside
 * [data_offset, data_offset + data_size) is read and a truncated image decodes as under AADHip_DecodePlanRun.  Per stream
 * bits_per_sample (2 / 3 / 4), block_size, num_samples_per_block and ch_process_method may differ; the channel count may not
 * (the output has one C), nor may has_file_header.  formats[i].num_samples is ignored: the lengths come from the table.
 *
 * Errors.  AAD_APIRESULT_INVALID_ARGUMENT for null pointers (streams and formats may be null while num_streams == 0),
 * num_channels outside 1 .. AAD_HIP_MAX_NUM_CHANNELS and any formats[i].num_channels != num_channels; otherwise every formats[i]
 * with streams[i] is validated exactly as AADHip_DecodePlanCreate validates its one format, stream by stream in order (the
 * channel count first), and the first failing stream's error is returned.  num_streams == 0 is OK: every window is zero.
 *
 * A run is one kernel per (bits, mid/side) pair present in the plan - at most six for two channels, three otherwise; a plan whose
 * streams share a format runs one kernel.  Every launch walks all the windows and writes those of its own streams; every element
 * of the output is written exactly once per run.  The start event of AADHip_ContextSignalNextRun rides on the first kernel and
 * the stop event on the last.  The run's errors are AADHip_WindowDecodePlanRun's; the lane count that must fit 64 bits is that of
 * the largest launch, N * (ceil((T - 1) / spb) + 1) * C for the smallest spb of the plan. */
AADApiResult AADHip_MixedWindowDecodePlanCreate(
    struct AADHipContext *context, uint32_t num_channels, int32_t has_file_header,
    uint32_t num_streams, const struct AADHipStreamDesc *streams,
    const struct AADHeaderInfo *formats, /* host array, one per stream */
    struct AADHipWindowDecodePlan **plan);

/* Window decode over a corpus that mixes mono and stereo streams, into rows of one channel count.  A constructor of its own that
 * returns an ordinary window decode plan: AADHip_WindowDecodePlanRun, AADHip_WindowDecodePlanDestroy and
 * AADHip_ContextSignalNextRun work on it unchanged.
 *
 * Definition.  D_s is what AADHip_DecodePlanRun writes for stream s under formats[s] - after the inverse mid/side, so D_s[t][0]
 * is L and D_s[t][1] is R.  Per stream bits_per_sample, block_size, num_samples_per_block, ch_process_method and the channel
 * count C_s (1 or 2) may differ; has_file_header may not.  With C = out_channels, for window w = {stream, first_frame}, t < T
 * and f = first_frame + t, out[(w * C + c) * T + t] is
 *   C_s == C:                    D_s[f][c] - the mixed-format plan's rule;
 *   C_s == 1, C == 2:            D_s[f][0] in both rows;
 *   C_s == 2, C == 1, int16:     (L + R) >> 1 with an arithmetic shift, i.e. the floor of the mean: L = R = -32768 gives -32768,
 *                                a sum of -3 gives -2;
 *   C_s == 2, C == 1, float32:   (float)(L + R) * 2^-16, the exact mean (|L + R| <= 65536 is exact in float32).  It is NOT the
 *                                int16 down-mix divided by 32768: the half step is kept.
 * Samples with f >= num_samples are zero, a window with stream >= num_streams is all zero in all C rows, wrapped int64 values
 * give zeros and read nothing, no byte outside [data_offset, data_offset + data_size) is read, and a truncated image decodes as
 * under AADHip_DecodePlanRun before the mix is taken.  formats[i].num_samples is ignored: the lengths come from the table.
 *
 * Errors.  AAD_APIRESULT_INVALID_ARGUMENT for null pointers (streams and formats may be null while num_streams == 0),
 * out_channels outside {1, 2} and any formats[i].num_channels outside {1, 2}; otherwise every formats[i] with streams[i] is
 * validated exactly as AADHip_DecodePlanCreate validates its one format, stream by stream in order (the channel count first),
 * and the first failing stream's error is returned.  num_streams == 0 is OK: every window is zero.
 *
 * A run is one kernel per (source channels, bits, mid/side) present in the plan, in the order of the mixed-format plan's six
 * two-channel kernels, then mono 4-, 3- and 2-bit: at most nine.  Every launch walks all the windows, with lanes for its SOURCE
 * channel count, and writes those of its own streams; every element of the output is written exactly once per run.  The start
 * event of AADHip_ContextSignalNextRun rides on the first kernel and the stop event on the last.  The run's errors are
 * AADHip_WindowDecodePlanRun's with N * out_channels * T elements; the lane count that must fit 64 bits is that of the largest
 * launch, N * (ceil((T - 1) / spb) + 1) * C_s for a variant's source channel count and smallest spb. */
AADApiResult AADHip_ChannelMixWindowDecodePlanCreate(
    struct AADHipContext *context, uint32_t out_channels /* 1 or 2 */, int32_t has_file_header,
    uint32_t num_streams, const struct AADHipStreamDesc *streams,
    const struct AADHeaderInfo *formats, /* host array, one per stream; num_channels 1 or 2 each */
    struct AADHipWindowDecodePlan **plan);

/* Window decode with exact per-row level statistics, from the decode kernels themselves: what a data loader asks of a crop (is
 * it silent, what is its RMS, how many of its frames did the stream have) without a second pass over the rows - and, with
 * device_out == NULL, without the rows.  For all three kinds of window decode plan.
 *
 * Definition.  Let C be the plan's output channel count (num_channels; out_channels of a channel-mix plan).  For window
 * w = {stream, first_frame}, row r < C and t < T let v[w][r][t] be the int16 value that AADHip_WindowDecodePlanRun with
 * AAD_HIP_SAMPLE_INT16 writes to out[(w * C + r) * T + t] for the same plan, data and windows.  The record of row (w, r) is the
 * AADHipRowStats (below) at index w * C + r - a torch int64 [N, C, 4] tensor on the device IS the table - with
 *   sum_sq  = sum over t of v * v,   sum_abs = sum over t of |v|,   max_abs = max over t of |v| (0 when nothing contributes;
 *             32768 is reachable),
 *   count   = the number of t < T with stream < num_streams and first_frame + t < num_samples[stream], that is
 *             min(T, num_samples - first_frame): 0 for a stray window or a wrapped value and where first_frame >= num_samples.
 *             It comes from the stream table alone - a truncated image does not change it - and is the row's padding mask.
 * Consequences:
 *   - the statistics do not depend on sample_type.  A float32 row is v / 32768 exactly, with one exception: the float32 down-mix
 *     (C_s = 2, C = 1) keeps the half step in the row, and its statistics are still those of the int16 floor mix (L + R) >> 1;
 *   - a mono stream decoded into two rows gives two equal records;
 *   - |v| <= 32768 and T < 2^32, so sum_sq <= 2^62: nothing wraps and every field is non-negative as int64;
 *   - the sums are integers, so two runs give the same bits whatever order the lanes finish in.
 *
 * Outputs.  The rows are byte for byte what AADHip_WindowDecodePlanRun writes; no other element of device_out and nothing outside
 * the N * C records is touched; every record is written, whatever the table held before.  device_out may be NULL: statistics only,
 * no row is written (and nothing is stored but the records).
 *
 * Errors.  AADHip_WindowDecodePlanRun's, except that a null device_out is allowed (sample_type is validated all the same), plus
 * AAD_APIRESULT_INVALID_ARGUMENT for a device_stats that is null or not 8-byte aligned while num_windows > 0 and for N * C * 32
 * bytes overflowing 64 bits (with T < 8 that can happen where N * C * T * 4 does not).  num_windows == 0 is OK and launches
 * nothing.
 *
 * The lanes of a row's blocks add into its record, so the run first clears the table on the context's stream and then launches
 * AADHip_WindowDecodePlanRun's kernels (same lanes, same variants).  AADHip_ContextSignalNextRun: the start event is recorded in
 * front of the clear - the run's first device operation - and the stop event rides on the run's last kernel. */
struct AADHipRowStats;
AADApiResult AADHip_WindowDecodePlanRunStats(
    struct AADHipWindowDecodePlan *plan, const uint8_t *device_data,
    uint64_t num_windows, const struct AADHipWindow *device_windows,
    uint32_t frames_per_window, int32_t sample_type,
    void *device_out,                     /* may be NULL: statistics only, no row is written */
    struct AADHipRowStats *device_stats); /* N * C records, 8-byte aligned, every one written by the run */

/* Window decode with a gain per window, written or added into float rows: what a loader does with the levels above - speech plus
 * noise at a chosen SNR, level normalisation, mixup, polarity flips - without a multiply pass over each batch and an add pass over
 * both.  A noisy batch is two runs into one buffer: STORE of g_s * speech, then ADD of g_n * noise.  For all three kinds of window
 * decode plan; asynchronous on the context's stream.  The gain table stays on the device and the host never reads it, exactly like
 * the window table (a contiguous torch float32 tensor [N] on the device IS the table).
 *
 * Definition.  IEEE arithmetic and nothing else.  For each element let f be the float32 value an AAD_HIP_SAMPLE_FLOAT32 run of
 * AADHip_WindowDecodePlanRun writes for the same plan, data and windows: sample * 2^-15, (L + R) * 2^-16 for the channel-mix
 * down-mix, +0 for every frame the stream does not produce, for stray windows and for wrapped values.  Let g = device_gain[w], one
 * gain for all rows of window w; 1.0f with a NULL table.  Let p = fl32(g * f): ONE float32 multiply, round to nearest even,
 * subnormal results kept - f is formed first, which is exact, then multiplied; (sample * g) * 2^-15 rounds twice once the result is
 * subnormal and is not the definition.  The element becomes
 *                                float32 rows                     float16 / bfloat16 rows
 *   AAD_HIP_WINDOW_GAIN_STORE    p                                p rounded once to the type, nearest even, subnormals kept
 *   AAD_HIP_WINDOW_GAIN_ADD      fl32(old + p)                    fl32(float32(old) + p) rounded once to the type
 * with old the element's content before the run.  The multiply and the add are two roundings, never a fused multiply-add, and a
 * 2-byte row is never rounded from a product that skipped its float32 rounding.  That is torch's
 * (out.float() + gain[:, None, None] * row_float32).to(dtype) for ADD and the same without `out.float() +` for STORE, evaluated on
 * every element of the N x C x T output, padding included.  Consequences:
 *   - a negative gain turns a zero sample, or padding, into -0 under STORE;
 *   - under ADD padding changes nothing, except that an old -0 plus +0 becomes +0;
 *   - every element is read at most once (ADD) and written exactly once per run, by one lane: a run is deterministic, and
 *     device_out may hold anything before a STORE run;
 *   - non-finite gains follow IEEE: NaN where f = 0, infinities elsewhere.  NaN payloads are unspecified;
 *   - a NULL table under STORE writes byte for byte what AADHip_WindowDecodePlanRun writes.
 *
 * Errors.  AADHip_WindowDecodePlanRun's, plus AAD_APIRESULT_INVALID_ARGUMENT for AAD_HIP_SAMPLE_INT16 (a gain on integer rows
 * needs a rounding and clipping rule, which only AADHip_SpectrogramRunMix states), a mode outside {0, 1} and a device_gain that
 * is not 4-byte aligned.  num_windows == 0 is OK and launches nothing.  A refused run writes nothing.
 *
 * There is no statistics variant: the levels are needed before the gains exist, so they come from a statistics-only
 * AADHip_WindowDecodePlanRunStats (device_out == NULL) first.
 *
 * The run launches the kernels AADHip_WindowDecodePlanRun launches for the plan - same lanes, same variants, same launch plan -
 * with the gain in the row writer.  AADHip_ContextSignalNextRun: the start event rides on the first kernel, the stop event on the
 * last. */
enum AADHipWindowGainMode {
  AAD_HIP_WINDOW_GAIN_STORE = 0, /* the element becomes g * f */
  AAD_HIP_WINDOW_GAIN_ADD = 1    /* the element becomes old + g * f */
};
AADApiResult AADHip_WindowDecodePlanRunGain(
    struct AADHipWindowDecodePlan *plan, const uint8_t *device_data,
    uint64_t num_windows, const struct AADHipWindow *device_windows,
    uint32_t frames_per_window, int32_t sample_type, void *device_out,
    const float *device_gain, /* num_windows floats on the device, 4-byte aligned; NULL: every gain is 1 */
    int32_t mode);            /* enum AADHipWindowGainMode */

/* Window decode with a span per window: a crop of L frames that starts at element o of its row instead of filling it - a noise
 * event, a second talker or an impulse shorter than the row, added at a random offset into a batch that is already there; a
 * variable-length utterance with zeros behind it, or in front of it for centred and right-aligned padding and random time shifts;
 * and the level of the L frames alone, which the SNR of an event needs.  For all three kinds of window decode plan; asynchronous
 * on the context's stream.  The span table stays on the device and the host never reads it, exactly like the window table.
 *
 * Definition.  T = frames_per_window, (L, o) = the span of window w; a NULL table: every span is (T, 0).
 *   Le = 0 if o >= T, else min(L, T - o)  - the comparison first: no sum of two 64-bit values is formed, huge and wrapped int64
 *   values are not an error.
 * Let f[c][i] be the float32 value AADHip_WindowDecodePlanRun with AAD_HIP_SAMPLE_FLOAT32 writes to element i of row c for the same
 * plan, data and window {stream, first_frame}: +0 past num_samples, for stray windows and for wrapped values included, and
 * (L + R) * 2^-16 for the down-mix.  Let g = device_gain[w] (1 with NULL) and p = fl32(g * f), exactly as in
 * AADHip_WindowDecodePlanRunGain.
 *   Inside the span, o <= t < o + Le:   STORE  the element becomes p[c][t - o]
 *                                       ADD    the element becomes fl32(old + p[c][t - o])
 *     then rounded once to the row's type; the multiply and the add are two roundings, never a fused multiply-add.
 *   Outside the span:                   STORE  the element becomes +0 - not g * 0: a negative gain gives no -0 there
 *                                       ADD    the element is neither read nor written: an old -0 stays -0, a NaN keeps its bits
 * In torch, per window: row = zeros (STORE) or out[w] (ADD), then
 *   row[:, o:o+Le] = (row[:, o:o+Le].float() + g * row_float32[:, :Le]).to(dtype)        without `row.float() +` under STORE.
 * Every element is written at most once per run, by one lane, under STORE exactly once: a run is deterministic.  With NULL spans,
 * or (T, 0) in every record, the bytes are those of AADHip_WindowDecodePlanRunGain.
 *
 * Statistics (AADHip_WindowDecodePlanRunPlacedStats): records only, no rows.  With v the int16 value of
 * AADHip_WindowDecodePlanRunStats' definition at crop index i, sum_sq, sum_abs and max_abs run over i < Le, and
 * count = min(Le, num_samples - first_frame): 0 for a stray window, a wrapped value or first_frame >= num_samples.  Every one of
 * the N * C records is written; the run clears the table first - AADHip_ContextSignalNextRun's start event sits in front of the
 * clear, its stop event rides on the last kernel.  With NULL spans the table is that of AADHip_WindowDecodePlanRunStats with
 * device_out == NULL.
 *
 * Errors.  Those of AADHip_WindowDecodePlanRunGain (AAD_HIP_SAMPLE_INT16 refused included) and of
 * AADHip_WindowDecodePlanRunStats respectively, plus AAD_APIRESULT_INVALID_ARGUMENT for a device_spans that is not 8-byte
 * aligned.  num_windows == 0 is OK and launches nothing.  A refused run writes nothing.
 *
 * Out of scope, deliberately: int16 rows; a run with both rows and statistics (the levels come first, as for the gain run); more
 * than one span per row in a run - several events in one row are several ADD runs; a span that loops a short stream.
 *
 * The run launches the kernels, lanes and launch plans of the run without spans for the same T; under STORE the K lanes of a
 * window share the zeros outside its span, each the tile it owns in a run without spans. */
struct AADHipWindowSpan {   /* a contiguous torch int64 [N, 2] tensor on the device IS the table */
  uint64_t num_frames;      /* L: frames of the crop */
  uint64_t out_frame;       /* o: row element that receives frame first_frame */
};
AADApiResult AADHip_WindowDecodePlanRunPlaced(
    struct AADHipWindowDecodePlan *plan, const uint8_t *device_data,
    uint64_t num_windows, const struct AADHipWindow *device_windows,
    const struct AADHipWindowSpan *device_spans,   /* NULL: every span is (T, 0) */
    uint32_t frames_per_window, int32_t sample_type, void *device_out,
    const float *device_gain, int32_t mode);
AADApiResult AADHip_WindowDecodePlanRunPlacedStats(
    struct AADHipWindowDecodePlan *plan, const uint8_t *device_data,
    uint64_t num_windows, const struct AADHipWindow *device_windows,
    const struct AADHipWindowSpan *device_spans,   /* NULL: every span is (T, 0) */
    uint32_t frames_per_window, struct AADHipRowStats *device_stats);

/* ---- resample: window decode at another rate, per-window rational ratio, exact integer FIR --------------------------------- */

/* A corpus holds files of several sampling rates, and speed perturbation draws a rate per window.  A resampler is a stage of its
 * own behind AADHip_WindowDecodePlanRun, for plans of all three constructors: a resolve kernel moves every window to the front by
 * the filter's lead, the window decode writes an int16 SOURCE BATCH of T_src frames per row, and a FIR kernel turns each source
 * row into T output frames at the window's own ratio.  The decode kernels are the ones of a plain run; the price is one int16
 * write and read per source sample.  Measured on MI355X, 1024 stereo windows of 48 000 frames at 147/160 into float32 rows:
 * resolve 0.006 ms, decode 0.146 ms, FIR 0.451 ms (1.35 TB/s moved), against 0.243 ms for a plain float32 decode of the same
 * windows - the FIR kernel, not the extra batch, is the cost (DESIGN.md "Window decode at another rate").  All arithmetic is
 * integer, so the rows are defined bit for bit.
 *
 * Ratio.  {up, down} is output rate / source rate, reduced by its gcd to (L, M).
 *
 * Bank of (L, M): L phases of K int16 taps in Q14.  (1, 1): K = 2, taps {16384, 0}.  Otherwise s = min(1, L / M),
 * K = 2 ceil(12 / s), and tap k of phase p sits at t = k - (K/2 - 1) - p / L with
 *   g = 0.94 s sinc(0.94 s t) I0(9 sqrt(1 - (t / (K/2))^2)) / I0(9),   sinc(x) = sin(pi x) / (pi x),   0 where |t| > K/2:
 * a Kaiser-windowed low-pass at 0.94 of the lower rate's Nyquist frequency, twelve zero crossings a side.  The phase is scaled to
 * sum to 16384 and floored, and the 16384 - sum(floors) taps with the largest fractional parts get 1 more, ties to the lower k:
 * every phase sums to exactly 16384, a constant stays a constant.  The bank is built on the host in double precision;
 * AADHip_ResamplerBank returns it (coefficients: L * K values, phase p's taps at p * K; NULL asks for L, M and K alone;
 * AAD_APIRESULT_INSUFFICIENT_BUFFER when capacity, in values, is below L * K).
 *
 * Row.  Window w = {stream, first_frame}, x the stream's decode (D_s of "window decode", any channel of the plan's rows), zero
 * before frame 0 and from num_samples on, (L, M, K, h) the window's bank.  For n < T, with i = (n M) div L and p = (n M) mod L:
 *   acc[n] = sum over k < K of h[p][k] * x[first_frame + i + k - (K/2 - 1)]
 * which int32 holds exactly, every phase having sum |h| <= 65535.  The element is
 *   INT16     clamp(floor((acc + 8192) / 16384), -32768, 32767)
 *   FLOAT32   fl32(acc) * 2^-29: the integer rounded to nearest even, then an exact scale
 *   FLOAT16 / BFLOAT16   that float32 value rounded once to nearest even, as for window decode rows
 * and with the (1, 1) bank bit for bit what AADHip_WindowDecodePlanRun writes for the window and type (a channel-mix plan's
 * stereo-to-mono rows are resampled as their int16 rows, (L + R) >> 1).
 *
 * Bank selection.  A resampler holds num_ratios ratios - bank r is ratio r's - and select[num_streams][variants] of bank indices,
 * 0xFFFF for none.  A run takes device_variant, int64[N] in device memory, NULL for all 0: window w's bank is
 * select[stream][variant[w]].  A stream index >= num_streams, a variant outside [0, variants) - negative ones included - and
 * 0xFFFF give a row of +0.  The host reads neither table.
 *
 * Source batch.  T_src = max over the banks of ((T - 1) M) div L + K (AADHip_ResamplerSourceFrames).  AADHip_ResamplerResolve
 * writes, per window, the source window {stream, src_first} with src_first = first_frame - min(first_frame, K/2 - 1), and the
 * lane record {bank, shift} with shift = first_frame - src_first.  The caller runs AADHip_WindowDecodePlanRun over the source
 * windows with frames_per_window = T_src and AAD_HIP_SAMPLE_INT16; element j of a source row is then frame src_first + j, and
 * AADHip_ResamplerRun reads j = shift + i + k - (K/2 - 1), 0 for j < 0.  Huge first_frame values pass through: window decode
 * makes their rows zeros.
 *
 * AADHip_ResamplerCreate: AAD_APIRESULT_INVALID_ARGUMENT for a null pointer, num_ratios == 0 or >= 0xFFFF, variants == 0, a
 * select entry that is neither a ratio's index nor 0xFFFF, and a ratio with up == 0 or down == 0, L > 1024, K > 256,
 * 2 L K > 65536 bytes or a phase with sum |h| > 65535.
 * AADHip_ResamplerResolve and AADHip_ResamplerRun are asynchronous on the context's stream, one kernel each; num_windows == 0
 * launches nothing and is OK; AADHip_ContextSignalNextRun's events are not theirs (the window decode between them takes them).
 * AAD_APIRESULT_INVALID_ARGUMENT: a null pointer (device_variant aside), a table off its alignment (8 bytes for windows and
 * variants, 4 for lanes, the element's for the rows), frames == 0 or (frames - 1) * M >= 2^31 for a bank, channels == 0,
 * source_frames below T_src, a sample_type other than the four of window decode, and N * C * T or N * C * source_frames elements
 * or bytes past 64 bits.  No refused call writes anything. */
struct AADHipResampleRatio {
  uint32_t up, down; /* output rate / source rate */
};
struct AADHipResampleLane { /* a contiguous torch int32 [N, 2] tensor on the device IS the table */
  uint32_t bank;            /* the window's bank, 0xFFFF: a row of zeros */
  uint32_t shift;           /* element of the source row that holds frame first_frame */
};
struct AADHipResampler;
AADApiResult AADHip_ResamplerCreate(
    struct AADHipContext *context, uint32_t num_ratios, const struct AADHipResampleRatio *ratios,
    uint32_t num_streams, uint32_t variants, const uint16_t *select,
    struct AADHipResampler **resampler);
void AADHip_ResamplerDestroy(struct AADHipResampler *resampler);
AADApiResult AADHip_ResamplerBank(
    const struct AADHipResampler *resampler, uint32_t ratio,
    uint32_t *L, uint32_t *M, uint32_t *taps, int16_t *coefficients, uint64_t capacity);
AADApiResult AADHip_ResamplerSourceFrames(
    const struct AADHipResampler *resampler, uint32_t frames, uint32_t *source_frames);
AADApiResult AADHip_ResamplerResolve(
    struct AADHipResampler *resampler, uint64_t num_windows, const struct AADHipWindow *device_windows,
    const int64_t *device_variant,   /* NULL: every variant is 0 */
    uint32_t frames, struct AADHipWindow *device_source_windows, struct AADHipResampleLane *device_lanes);
AADApiResult AADHip_ResamplerRun(
    struct AADHipResampler *resampler, uint64_t num_windows, uint32_t channels,
    const int16_t *device_source_rows, uint32_t source_frames, const struct AADHipResampleLane *device_lanes,
    uint32_t frames, int32_t sample_type, void *device_out);

/* A wide resampler: ratios whose bank does not fit a workgroup's LDS.  16 kHz rows from a 44.1 kHz stream at speeds 9/10 and 11/10
 * are the ratios 1600/3969 and 1600/4851, 48 kHz rows from it at 11/10 are 1600/1617: L = 1600, which AADHip_ResamplerCreate
 * refuses.  AADHip_ResamplerCreateWide takes AADHip_ResamplerCreate's arguments and returns an ordinary resampler:
 * AADHip_ResamplerBank, ...SourceFrames, ...Resolve, ...Run, ...RunGain, ...RunStats and ...Destroy take it as they take any other,
 * with their own errors, and every definition above and below - the bank, the row, the resolve, T_src, the spans, the records -
 * holds for it word for word.  Only the limits of a ratio differ, after reduction:
 *   L <= 32768, K <= 256 (as before), 2 L K <= 2 MiB per bank, sum |h| <= 65535 per phase (as before), and fewer than 2^31
 *   coefficients in all banks together, a bank that AADHip_ResamplerCreate would refuse counted with K rounded up to 8;
 * every other refusal - null pointers, num_ratios, variants, select entries, up == 0 or down == 0 - is AADHip_ResamplerCreate's.
 * Opt-in: AADHip_ResamplerCreate keeps its limits, its refusals and its kernels.  The runs of a wide resampler launch kernels of
 * their own, which keep a bank that AADHip_ResamplerCreate would accept whole in LDS - its rows are then computed by the same
 * code, the same bits follow from the definition either way - and read only the bank rows a round of 64 to 256 consecutive
 * outputs uses from global memory for any other (DESIGN.md "Wide resampler").  Banks are built on the host as before. */
AADApiResult AADHip_ResamplerCreateWide(
    struct AADHipContext *context, uint32_t num_ratios, const struct AADHipResampleRatio *ratios,
    uint32_t num_streams, uint32_t variants, const uint16_t *select,
    struct AADHipResampler **resampler);

/* Resampled rows with a gain, spans and level statistics: the loader toolbox of window decode - AADHip_WindowDecodePlanRunStats,
 * ...RunGain, ...RunPlaced, ...RunPlacedStats - in the FIR kernel, for the corpus whose speech and noise come at different rates.
 * A noisy batch at one output rate decodes each source batch once (AADHip_ResamplerResolve, then
 * AADHip_WindowDecodePlanRunStats with AAD_HIP_SAMPLE_INT16 over the source windows) and runs the FIR over it twice: statistics
 * only for the levels, then STORE of the speech and ADD of gain * noise.  Both calls take AADHip_ResamplerRun's source rows and
 * lanes, are asynchronous on the context's stream and leave AADHip_ContextSignalNextRun's events alone.
 *
 * Spans are in OUTPUT frames: T = frames, (L, o) = device_spans[w], a NULL table: every span is (T, 0), and
 *   Le = 0 if o >= T, else min(L, T - o)  - the rule of "window decode with spans", the comparison first.
 *
 * Rows of AADHip_ResamplerRunGain.  Let f[c][n] be the float32 element AADHip_ResamplerRun writes with AAD_HIP_SAMPLE_FLOAT32 for
 * the same source rows and lanes: fl32(acc[n]) * 2^-29, +0 for a window without a bank.  Everything else is the text of "window
 * decode with spans" with this f in place of the window decode's value: g = device_gain[w] (1 with NULL), p = fl32(g * f) - ONE
 * float32 multiply of the finished f - and
 *   inside the span, o <= t < o + Le:   STORE  the element becomes p[c][t - o]
 *                                       ADD    the element becomes fl32(old + p[c][t - o]), a second rounding, never an fma
 *     then rounded once to a 2-byte type;
 *   outside the span:                   STORE  the element becomes +0 - not g * 0
 *                                       ADD    the element is neither read nor written.
 * A window without a bank has f = +0: STORE gives g * 0 inside the span (-0 under a negative gain, as the gain definition says
 * for padding) and +0 outside, ADD gives old + g * 0 inside.  Every element is written at most once per run, by one thread, under
 * STORE exactly once: device_out may hold anything before a STORE run, rows with Le = 0 included.  With NULL spans, a NULL gain
 * and STORE the bytes are those of AADHip_ResamplerRun.
 *
 * Records of AADHip_ResamplerRunStats.  Let v[c][n] be the int16 element AADHip_ResamplerRun writes with AAD_HIP_SAMPLE_INT16 -
 * whatever sample_type the run has.  Record w * C + c holds
 *   sum_sq = sum of v^2, sum_abs = sum of |v|, max_abs = max of |v|, each over n < Le - filter tails past the stream's end are
 *            part of the row and count into the sums;
 *   count  = 0 when c' <= shift, else min(Le, ceil((c' - shift) L / M)), with c' = min(device_source_stats[w * C + c].count,
 *            source_frames) and {bank, shift} the window's lane: the number of n < Le whose centre source frame, element
 *            shift + (n M) div L of the source row, the stream had.  It is the row's padding mask.
 * A window without a bank gets an all-zero record.  Consequence: when the source batch was decoded over AADHip_ResamplerResolve's
 * source windows with statistics, count equals the number of n < Le with first_frame + (n M) div L < num_samples[stream].  The
 * sums are integers: two runs give the same bits.  Rows, when device_out is not NULL, are byte for byte AADHip_ResamplerRun's.
 * The run clears the N * C records on the context's stream, then launches one kernel; every record is written, whatever the
 * table held before.
 *
 * Errors.  AADHip_ResamplerRun's - with device_out == NULL too: sample_type is validated all the same, and N * C * T elements or
 * bytes of that type past 64 bits are refused although no row is written - plus AAD_APIRESULT_INVALID_ARGUMENT
 * for AAD_HIP_SAMPLE_INT16 in the gain run (as for window decode), a mode outside {0, 1}, a device_gain that is not 4-byte
 * aligned, a device_spans, device_stats or device_source_stats that is not 8-byte aligned, a null device_stats or
 * device_source_stats while num_windows > 0, device_out != NULL together with device_spans != NULL in the statistics run (no
 * run with both placed rows and statistics, as for window decode) and N * C * 32 bytes overflowing 64 bits.  num_windows == 0 is
 * OK and launches nothing.  A refused run writes nothing.
 *
 * Out of scope, deliberately: int16 rows with a gain, placed rows together with statistics, several spans per row in one run. */
AADApiResult AADHip_ResamplerRunGain(
    struct AADHipResampler *resampler, uint64_t num_windows, uint32_t channels,
    const int16_t *device_source_rows, uint32_t source_frames, const struct AADHipResampleLane *device_lanes,
    const struct AADHipWindowSpan *device_spans,   /* NULL: every span is (T, 0); in OUTPUT frames */
    uint32_t frames, int32_t sample_type, void *device_out,
    const float *device_gain,                      /* NULL: every gain is 1 */
    int32_t mode);                                 /* enum AADHipWindowGainMode */
AADApiResult AADHip_ResamplerRunStats(
    struct AADHipResampler *resampler, uint64_t num_windows, uint32_t channels,
    const int16_t *device_source_rows, uint32_t source_frames, const struct AADHipResampleLane *device_lanes,
    const struct AADHipRowStats *device_source_stats, /* N * C records: what AADHip_WindowDecodePlanRunStats wrote for the source batch */
    const struct AADHipWindowSpan *device_spans,   /* NULL: every span is (T, 0); in OUTPUT frames */
    uint32_t frames, int32_t sample_type,
    void *device_out,                              /* may be NULL: statistics only */
    struct AADHipRowStats *device_stats);          /* N * C records, every one written */

/* ---- reverberation: decoded windows convolved with impulse responses, exact integer FIR on the matrix cores ------------------ */

/* The third waveform augmentation of a loader, beside speed perturbation (the resample stage) and additive noise (the gain runs):
 * each crop convolved with a room impulse response drawn per window.  A convolver is a stage of the resample stage's shape: a
 * resolve kernel moves every window to the front by the response's lead, the plan's own window decode writes an int16 SOURCE
 * BATCH of T_src frames per row, and a FIR kernel turns each source row into T output frames through the row writers of the
 * resample stage.  A response has thousands of taps, so the sums run as int8 matrix products (DESIGN.md "Reverberation"); all
 * arithmetic is integer and the rows are defined bit for bit.
 *
 * Response r of a convolver: K_r int16 taps h_r[k], 1 <= K_r <= 32768, a scale exponent q_r in 0..15 and a delay d_r in
 * 0..K_r - 1, built on the host from float32 taps h (aad_convolve.h):
 *   h_q[k] = rint(h[k] * 2^q), ties to even, the product formed in double (exact); q is the largest value in 0..15 with
 *   max |h_q| <= 32639 - the bound under which every tap splits into two signed bytes - and 15 for an all-zero response;
 *   d_r is delays[r] when delays is not NULL and delays[r] >= 0, else the index of the largest |h_q|, the lowest on ties: the
 *   direct path, so that the reverberant row stays time-aligned with the dry one.  lead_r = K_r - 1 - d_r.
 * AADHip_ConvolverResponse returns K, q, the delay and the taps (taps: K values; NULL asks for the three numbers alone;
 * AAD_APIRESULT_INSUFFICIENT_BUFFER when capacity, in values, is below K).
 *
 * Row.  Window w = {stream, first_frame} with response r = response[w], x the stream's decode (one channel row of the plan), zero
 * before frame 0 and from num_samples on.  For n < T:
 *   acc[n] = sum over k < K_r of h_r[k] * x[first_frame + n + d_r - k]
 * an exact integer, |acc| < 2^45, held in 64 bits; the same response is applied to every channel row.  With Q = q_r the element is
 *   INT16     clamp(floor((acc + (Q ? 2^(Q-1) : 0)) / 2^Q), -32768, 32767)
 *   FLOAT32   fl32(acc) * 2^-(15 + Q): the 64-bit integer rounded once to nearest even, then an exact scale
 *   FLOAT16 / BFLOAT16   that float32 value rounded once to nearest even, as for window decode rows
 * With the response {1.0} the taps are {16384}, Q = 14, and the rows are bit for bit AADHip_WindowDecodePlanRun's.
 *
 * Selection.  device_response is int64[N] in device memory, never read on the host; NULL: every window uses response 0.  An index
 * outside [0, R), negative ones included, gives a row of +0; a stream index the plan does not have gives a row of +0 as well (its
 * source row is zeros).
 *
 * Source batch.  T_src = T + max_r K_r - 1 (AADHip_ConvolverSourceFrames).  AADHip_ConvolverResolve writes, per window, the source
 * window {stream, src_first} with src_first = first_frame - min(first_frame, lead_r) and the lane record {response, shift} with
 * shift = first_frame - src_first; a window without a response keeps its start and gets response 0xFFFFFFFF.  The caller runs
 * AADHip_WindowDecodePlanRun over the source windows with frames_per_window = T_src and AAD_HIP_SAMPLE_INT16, and
 * AADHip_ConvolverRun reads source element j = shift + n + d_r - k, 0 for j < 0.  Huge and wrapped first_frame values pass
 * through, as for AADHip_ResamplerResolve.
 *
 * AADHip_ConvolverRunGain: the definitions of "Resampled rows with a gain, spans and level statistics", word for word, with f the
 * FLOAT32 element above: p = fl32(g * f), one float32 multiply; ADD is a second rounding, never an fma; Le by the rule of window
 * decode with spans, in output frames; STORE writes +0 outside the span, ADD touches nothing there; float rows only.
 *
 * AADHip_ConvolverCreate: AAD_APIRESULT_INVALID_ARGUMENT for a null pointer, num_responses == 0, a length outside 1..32768, a tap
 * that is not finite or misses the bound even at q = 0, and a delay >= K.  Resolve and the runs are asynchronous on the context's
 * stream, one kernel each; num_windows == 0 launches nothing and is OK.  They refuse what AADHip_ResamplerResolve and
 * AADHip_ResamplerRun / ...RunGain refuse: a null pointer (device_response, device_spans and device_gain aside), a table off its
 * alignment, frames == 0, channels == 0, source_frames below T_src, an unknown sample type, int16 rows or a mode outside {0, 1}
 * in the gain run, and extents past 64 bits.  No refused call writes anything.
 *
 * Records of AADHip_ConvolverRunStats: the last tool of the loader toolbox, for speech convolved with a room response and noise
 * added at an SNR measured against the REVERBERANT speech.  The call takes AADHip_ResamplerRunStats' twelve arguments with the
 * convolver's types; the record is struct AADHipRowStats, unchanged.  Let v[c][n] be the INT16 element above - whatever
 * sample_type the run has.  Record w * C + c holds
 *   sum_sq = sum of v^2, sum_abs = sum of |v|, max_abs = max of |v|, each over n < Le, Le by the rule of window decode with spans
 *            in output frames, a NULL table: every span is (T, 0) - the reverberant tail behind the stream's end is part of the
 *            row and counts into the sums;
 *   count  = 0 when c' <= shift, else min(Le, c' - shift), in 64 bits, with c' = min(device_source_stats[w * C + c].count,
 *            source_frames) and shift the window's lane field: the number of n < Le whose direct-path source element, shift + n,
 *            the stream had (convolve_output_count, aad_convolve.h).
 * Consequence: when the source batch was decoded with statistics over AADHip_ConvolverResolve's source windows, count equals the
 * number of n < Le with first_frame + n < num_samples[stream] - the padding mask of the DRY row; the delay keeps the reverberant
 * row aligned with it.  A window without a response gets an all-zero record, and rows of +0 where rows are asked for.  Rows,
 * when device_out is not NULL, are byte for byte AADHip_ConvolverRun's.  The run clears the N * C records on the context's stream,
 * then launches one kernel; every record is written, whatever the table held before.  The sums are integers: two runs give the
 * same bits.
 * The statistics are those of the INT16 row.  A float row that passes full scale is not clamped, but its record is - a response
 * normalised in energy can do that - and a max_abs of 32767 or 32768 is the witness of a clipped record.  It is the resample
 * stage's rule, kept so that level_dbfs, rmse and snr_gains stay in int16 units everywhere; an unclamped v^2 would not fit the
 * record either: |acc| / 2^Q reaches 2^45.
 * Refusals: exactly those of AADHip_ResamplerRunStats - a null or 8-byte-unaligned device_stats or device_source_stats while
 * num_windows > 0, a device_spans off 8-byte alignment, device_out != NULL together with device_spans != NULL, N * C * 32 bytes
 * past 64 bits, and everything AADHip_ConvolverRun refuses, with device_out optional (sample_type and the extents of the rows
 * are validated all the same).  num_windows == 0 is OK and launches nothing.  A refused run writes nothing.
 *
 * Out of scope, deliberately: a response per channel, responses past 32768 taps. */
struct AADHipConvolveLane { /* a contiguous torch int32 [N, 2] tensor on the device IS the table */
  uint32_t response;        /* the window's response, 0xFFFFFFFF: a row of zeros */
  uint32_t shift;           /* element of the source row that holds frame first_frame */
};
struct AADHipConvolver;
AADApiResult AADHip_ConvolverCreate(
    struct AADHipContext *context, uint32_t num_responses, const float *const *taps, const uint32_t *lengths,
    const int32_t *delays,           /* NULL, or -1 for a response: the peak */
    struct AADHipConvolver **convolver);
void AADHip_ConvolverDestroy(struct AADHipConvolver *convolver);
AADApiResult AADHip_ConvolverResponse(
    const struct AADHipConvolver *convolver, uint32_t response,
    uint32_t *num_taps, uint32_t *scale, uint32_t *delay, int16_t *taps, uint64_t capacity);
AADApiResult AADHip_ConvolverSourceFrames(
    const struct AADHipConvolver *convolver, uint32_t frames, uint32_t *source_frames);
AADApiResult AADHip_ConvolverResolve(
    struct AADHipConvolver *convolver, uint64_t num_windows, const struct AADHipWindow *device_windows,
    const int64_t *device_response,  /* NULL: every window uses response 0 */
    uint32_t frames, struct AADHipWindow *device_source_windows, struct AADHipConvolveLane *device_lanes);
AADApiResult AADHip_ConvolverRun(
    struct AADHipConvolver *convolver, uint64_t num_windows, uint32_t channels,
    const int16_t *device_source_rows, uint32_t source_frames, const struct AADHipConvolveLane *device_lanes,
    uint32_t frames, int32_t sample_type, void *device_out);
AADApiResult AADHip_ConvolverRunGain(
    struct AADHipConvolver *convolver, uint64_t num_windows, uint32_t channels,
    const int16_t *device_source_rows, uint32_t source_frames, const struct AADHipConvolveLane *device_lanes,
    const struct AADHipWindowSpan *device_spans,   /* NULL: every span is (T, 0); in output frames */
    uint32_t frames, int32_t sample_type, void *device_out,
    const float *device_gain,                      /* NULL: every gain is 1 */
    int32_t mode);                                 /* enum AADHipWindowGainMode */
AADApiResult AADHip_ConvolverRunStats(
    struct AADHipConvolver *convolver, uint64_t num_windows, uint32_t channels,
    const int16_t *device_source_rows, uint32_t source_frames, const struct AADHipConvolveLane *device_lanes,
    const struct AADHipRowStats *device_source_stats, /* N * C records: what AADHip_WindowDecodePlanRunStats wrote for the source batch */
    const struct AADHipWindowSpan *device_spans,   /* NULL: every span is (T, 0); in output frames */
    uint32_t frames, int32_t sample_type,
    void *device_out,                              /* may be NULL: statistics only */
    struct AADHipRowStats *device_stats);          /* N * C records, every one written */

/* ---- spectrogram: int16 rows to power-spectrum or filterbank energies, exact integer DFT on the matrix cores ------------------ */

/* The last step of a loader for models that read log-mel features: any int16 row batch on the device - a window decode's, a
 * resampler's or a convolver's (sample type INT16) - framed, windowed, transformed and, with filters, reduced to filterbank
 * energies by ONE kernel, with no float32 batch, no complex spectrum and no elementwise pass.  Every element is defined bit for
 * bit, like every other stage's.
 *
 * Parameters.  n_fft with 1 <= win_length W <= n_fft <= 4096; hop H >= 1; window float32 [W], every value finite;
 *   B = n_fft / 2 + 1 bins; num_filters M >= 0 with filters float32 [M][B], dense and row-major, every weight finite, every
 *   nonzero weight of magnitude >= 2^-60 (no product below is subnormal), negative weights allowed; filters is NULL exactly when
 *   M = 0.
 * Coefficients.  In double, c[t][k] = (double)w[t] cos(2 pi ((k t) mod n_fft) / n_fft) and s[t][k] = -(double)w[t] sin(the same
 *   angle), t < W, k < B, the reduction (k t) mod n_fft in integers.  Both matrices are quantised together by the convolver's
 *   rule: cq = rint(c 2^q), sq = rint(s 2^q), ties to even, q the largest of 0..15 with max |.| <= 32639; Create refuses a
 *   window for which q = 0 does not fit.  AADHip_SpectrogramCoefficients returns q and both matrices.
 * Frames.  A row of T elements gives F = 1 + (T - W) / H frames (floor); T < W is refused.  No centring, no padding: a caller
 *   who wants a centred frame starts the window earlier.
 * Sums.  Re[f][k] = sum over t < W of x[f H + t] cq[t][k], Im[f][k] likewise with sq: exact integers below 2^42 in magnitude.
 * Elements.  re = fl32(Re) 2^-(15 + q) - the 64-bit integer rounded once to nearest even, then an exact scale, the convolver's
 *   FLOAT32 rule - im likewise, and P[f][k] = fl32(fl32(re re) + fl32(im im)): two multiplies and one add, never a fused one.
 *   The units are those of a waveform in [-1, 1) under an unnormalised DFT: what torch.stft(center=False) followed by
 *   abs() ** 2 approximates.
 * Filters.  lo_j and hi_j are the indices of filter j's first and last nonzero weight.  E[f][j] starts at +0 and, for
 *   k = lo_j, lo_j + 1, ..., hi_j in that order, E = fl32(E + fl32(filters[j][k] P[f][k])); a zero inside the band is multiplied
 *   like any other weight; an all-zero filter gives +0.
 * Output.  float32, contiguous: [num_rows, F, M] for M > 0, and [num_rows, F, B], P itself, for M = 0.  Two runs give the same
 *   bits.
 *
 * The coefficients are int16 because the rows are decodes of a 2- to 4-bit codec, whose error lies orders of magnitude above a
 * 2^-15 coefficient rounding; the price shows on a pure full-scale tone, where bands some 90 dB below the peak are coefficient
 * noise (DESIGN.md "Spectrogram" has the measured floor).
 *
 * Not built: the logarithm (no correctly rounded log exists on the device, and one torch.log over an output 5 to 10 times smaller
 * than the waveform is cheap); float16 / bfloat16 outputs (pointless in front of the log); magnitude (power = 1); the [.., M, F]
 * layout (transpose(-1, -2) is a view); pre-emphasis, dither and DC removal; n_fft past 4096; coefficients wider than int16.
 *
 * Create returns AAD_APIRESULT_INVALID_ARGUMENT for anything the definition excludes.  Run is asynchronous on the context's
 * stream; num_rows == 0 launches nothing and returns OK.  Otherwise the calls refuse a null pointer, device_rows off 2-byte or
 * device_out off 4-byte alignment, frames < win_length, row_pitch < frames and extents past 64 bits; a refused call writes
 * nothing. */
struct AADHipSpectrogram;
AADApiResult AADHip_SpectrogramCreate(
    struct AADHipContext *context, uint32_t n_fft, uint32_t win_length, uint32_t hop, const float *window,
    uint32_t num_filters, const float *filters, /* NULL exactly when num_filters == 0 */
    struct AADHipSpectrogram **spectrogram);
void AADHip_SpectrogramDestroy(struct AADHipSpectrogram *spectrogram);
/* F of rows of `frames` elements */
AADApiResult AADHip_SpectrogramFrames(const struct AADHipSpectrogram *spectrogram, uint32_t frames, uint32_t *num_frames);
/* the scale exponent q and the quantised cos / -sin matrices, int16 [W][B][2]; cos_sin NULL: the scale alone.
 * AAD_APIRESULT_INSUFFICIENT_BUFFER for a capacity (in elements) below W * B * 2 */
AADApiResult AADHip_SpectrogramCoefficients(
    const struct AADHipSpectrogram *spectrogram, uint32_t *scale, int16_t *cos_sin, uint64_t capacity);
AADApiResult AADHip_SpectrogramRun(
    struct AADHipSpectrogram *spectrogram, uint64_t num_rows, const int16_t *device_rows,
    uint64_t row_pitch, /* in elements, >= frames */
    uint32_t frames, float *device_out);

/* Mix.  The spectrogram of a sum of two int16 row batches at gains - speech plus noise at an SNR - with the sum formed while the
 * kernel stages its samples: no float32 batch, no quantise pass.  Every other stage refuses a gain on int16 rows, because such a
 * gain needs a rounding and clipping rule; this is the one stage that asks for it, and here it is.
 *
 * Definition.  T = frames.  For row r let G = r / rows_per_gain, ga = device_gain_a[G], gb = device_gain_b[G] (1 with NULL) and
 * (L, o) = device_spans[G] ((T, 0) with NULL); Le follows "Window decode with a span": Le = 0 if o >= T, else min(L, T - o) - the
 * comparison first, so huge and wrapped values are no error.  For element j < T, with a and b the int16 values converted to
 * float32 exactly:
 *   Outside the span:                  m = fl32(ga a[j])
 *   Inside the span, o <= j < o + Le:  m = fl32(fl32(ga a[j]) + fl32(gb b[j - o]))  - two multiplies and one add, three
 *                                      roundings, never a fused multiply-add
 *   Quantise:                          x[j] = 0 if m is a NaN; else m rounded to the nearest integer, ties to even, and clamped
 *                                      to [-32768, 32767] - an infinite m gives the rail.
 * The output is, bit for bit, what AADHip_SpectrogramRun writes for a batch that holds x.  b is read only at indices below Le,
 * a only below T; a and b may be the same memory.
 *
 * Two identities.  With ga = 1 and products that do not underflow, x = clamp(rint(32768 f)), f the float32 element that a STORE
 * of a and an ADD of gb b with the same span write (AADHip_WindowDecodePlanRunPlaced): f = fl32(a 2^-15 + fl32(gb b 2^-15)), and
 * scaling by a power of two commutes with every rounding above the subnormals.  It does NOT hold where the channel-mix plan
 * down-mixes stereo to mono: the int16 row holds the floor of the mean, the float row the exact mean.
 *
 * No clip count is returned: a caller who must not clip bounds the peak with |ga| max_abs_a + |gb| max_abs_b from the statistics
 * tables' peak column.  Out of scope: more than two operands, a span for a, and gains on the int16 rows of any other stage.
 *
 * Refused, each writing nothing: everything AADHip_SpectrogramRun refuses, for both row pointers and both pitches;
 * rows_per_gain == 0 or num_rows not a multiple of it; a gain table off 4-byte or a span table off 8-byte alignment.
 * num_rows == 0 is OK and launches nothing. */
AADApiResult AADHip_SpectrogramRunMix(
    struct AADHipSpectrogram *spectrogram, uint64_t num_rows,
    const int16_t *device_rows_a, uint64_t row_pitch_a,
    const int16_t *device_rows_b, uint64_t row_pitch_b,
    uint32_t rows_per_gain,                                   /* C: rows that share one gain pair and one span */
    const float *device_gain_a, const float *device_gain_b,   /* num_rows / rows_per_gain floats each; NULL: every gain 1 */
    const struct AADHipWindowSpan *device_spans,              /* of b, num_rows / rows_per_gain records; NULL: (T, 0) */
    uint32_t frames, float *device_out);

/* ---- planar encode: int16 / float32 rows per channel into .aad images ------------------------ */

/* The write side of the planar layout window decode reads out: one row per channel, int16 or float32 - torch's [N, C, T] - encoded
 * by the encoder kernels themselves, with no interleaving or conversion pass in front.
 *
 * Definition.  For stream i (descriptor d_i), channel c < C and frame t < num_samples_i the input value is
 *   v = x[pcm_offset_i + c * channel_stride + t]        (offsets in elements of the sample type)
 * and the encoder sees the int16 sample q(v):
 *   int16:    q(v) = v
 *   float32:  q(v) = 0 if v is a NaN (quiet or signalling), else clamp(roundTiesToEven(v * 32768), -32768, 32767)
 *             (v * 32768 is exact in float32, or overflows to +-inf and clamps; as torch:
 *             nan_to_num(x, nan=0).mul(32768).round().clamp(-32768, 32767).to(int16).  q inverts window decode's float32 output.)
 * The image bytes are those AADHip_EncodePlanRun writes for a plan with the same parameter, descriptor table (data_offset,
 * data_size, num_samples), segmentation (NULL: AADHip_EncodePlanCreate, else AADHip_SegmentedEncodePlanCreate) and device_state,
 * run on the interleaved int16 buffer P_i[t * C + c] = q(v); M/S is formed from q(L) and q(R).  So without segmentation the bytes
 * are the reference encoder's, with it those of the segmented definition above.
 *
 * A planar plan is an ordinary AADHipEncodePlan: AADHip_EncodePlanDestroy destroys it, and AADHip_ContextSignalNextRun's events
 * ride on AADHip_PlanarEncodePlanRun's one kernel.  AADHip_EncodePlanRun refuses a planar plan and AADHip_PlanarEncodePlanRun an
 * interleaved one (AAD_APIRESULT_INVALID_ARGUMENT): neither misreads its input.  device_samples may sit at any element offset.
 * Errors are those of AADHip_EncodePlanCreate / AADHip_SegmentedEncodePlanCreate and AADHip_EncodePlanRun, plus
 * AAD_APIRESULT_INVALID_ARGUMENT for a null layout, an unknown sample_type or a non-zero reserved, C > 1 with channel_stride below
 * any stream's num_samples, and a stream whose last element (pcm_offset + (C - 1) channel_stride + num_samples) or its byte offset
 * overflows 64 bits. */
struct AADHipPlanarLayout {
  int32_t sample_type;     /* enum AADHipSampleType: AAD_HIP_SAMPLE_INT16 or AAD_HIP_SAMPLE_FLOAT32 */
  uint32_t reserved;       /* 0 */
  uint64_t channel_stride; /* elements from channel c's row of a stream to channel c + 1's (ignored for mono) */
};
AADApiResult AADHip_PlanarEncodePlanCreate(
    struct AADHipContext *context, const struct AADEncodeParameter *parameter,
    const struct AADHipPlanarLayout *layout,
    const struct AADHipSegmentation *segmentation, /* NULL: the serial (reference-exact) encode */
    uint32_t num_streams, const struct AADHipStreamDesc *streams,
    struct AADHipEncodePlan **plan);
AADApiResult AADHip_PlanarEncodePlanRun(
    struct AADHipEncodePlan *plan, const void *device_samples, uint8_t *device_data,
    struct AADHipLaneState *device_state);

/* ---- planar reconstruct: [N, C, T] rows through the codec in one kernel ---------------------------------------------------- */

/* A planar reconstruct plan is a planar encode plan with an output: "what do these rows sound like after the codec", with no
 * second recurrence - the decoder's output of an image is the encoder's own reconstruction, so the encoder kernels write it as
 * they encode.
 *
 * Definition.  Parameter, descriptor table, input layout (struct AADHipPlanarLayout), segmentation and state follow
 * AADHip_PlanarEncodePlanCreate / AADHip_PlanarEncodePlanRun.  A run
 *   1. writes into device_data exactly the bytes AADHip_PlanarEncodePlanRun writes for the same plan inputs, and
 *   2. for stream i, channel c < C and frame t < num_samples_i writes
 *        out[i * stream_stride + c * channel_stride + t] = D_i[t][c]   converted to the output sample type,
 *      D_i being what AADHip_DecodePlanRun writes for that image: int16 output is D_i[t][c], float32 output D_i[t][c] / 32768
 *      (exact, as window decode).
 * No other element of `out` is touched.  Input and output sample types are independent (int16 or float32 each).  Overlap of `out`
 * with the input or the images is undefined (device_out == device_samples is refused).
 * 2. also holds where a block header cannot carry the encoder's weights: a magnitude of 2^30 or more at a block start (a carried
 * record that starts there, or weights that grow past it) needs a weight shift of 16 and the header's 4-bit field wraps, as in the
 * reference built with NDEBUG; and a weight of INT32_MIN, which the shift ignores, reads back from its 16-bit field as 0.  A
 * decoder runs that block on the weights it reads, so D_i there is not the encoder's own reconstruction; the run compares every
 * header it writes with what a decoder reads back from it, walks such a block with the decoder's recurrence beside the encoder's
 * and writes D_i (and accounts for it in the statistics below).  tests/test_gpu_crafted_state.py.
 *
 * The plan is an ordinary AADHipEncodePlan: AADHip_EncodePlanDestroy destroys it, and AADHip_ContextSignalNextRun's events ride on
 * AADHip_PlanarReconstructPlanRun's one kernel.  AADHip_EncodePlanRun and AADHip_PlanarEncodePlanRun refuse it and
 * AADHip_PlanarReconstructPlanRun refuses every other plan (AAD_APIRESULT_INVALID_ARGUMENT).  The trial search always runs on the
 * single lane layout (AAD_HIP_OPTION_TRIAL_LANES does not apply); the bytes are the same either way.
 * Errors are those of AADHip_PlanarEncodePlanCreate / AADHip_PlanarEncodePlanRun, plus AAD_APIRESULT_INVALID_ARGUMENT for a null
 * `output`, an unknown output sample_type or a non-zero reserved, C > 1 with output channel_stride below the longest num_samples,
 * more than one stream with stream_stride < (C - 1) channel_stride + the longest num_samples (rows must not overlap), an end of the
 * rows ((N - 1) stream_stride + (C - 1) channel_stride + the longest num_samples) that overflows 64 bits in elements or bytes, and
 * from the run device_out == device_samples or a null device_out while the plan has streams. */
struct AADHipPlanarOutput {
  int32_t sample_type;     /* enum AADHipSampleType: AAD_HIP_SAMPLE_INT16 or AAD_HIP_SAMPLE_FLOAT32 */
  uint32_t reserved;       /* 0 */
  uint64_t stream_stride;  /* elements from stream i's channel-0 row to stream i + 1's */
  uint64_t channel_stride; /* elements from channel c's row to channel c + 1's (ignored for mono) */
};
AADApiResult AADHip_PlanarReconstructPlanCreate(
    struct AADHipContext *context, const struct AADEncodeParameter *parameter,
    const struct AADHipPlanarLayout *input, const struct AADHipPlanarOutput *output,
    const struct AADHipSegmentation *segmentation, /* NULL: the serial (reference-exact) encode */
    uint32_t num_streams, const struct AADHipStreamDesc *streams,
    struct AADHipEncodePlan **plan);
AADApiResult AADHip_PlanarReconstructPlanRun(
    struct AADHipEncodePlan *plan, const void *device_samples, uint8_t *device_data, void *device_out,
    struct AADHipLaneState *device_state);

/* ---- planar reconstruct statistics: exact per-row codec error from the same kernel ------------------------------------------- */

/* "How large is the error, per row?" - answered by the kernel that holds both operands anyway.
 *
 * Definition.  For a planar reconstruct plan (any input / output sample type, segmentation, state), stream i, channel c < C and
 * frame t < num_samples_i let
 *     e[i][c][t] = q(x[i][c][t]) - D_i[t][c]
 * q being the planar encode's input conversion (identity for int16; the float32 rule above AADHip_PlanarEncodePlanCreate) and D_i
 * what AADHip_DecodePlanRun gives for the image the run writes - the int16 value behind the row AADHip_PlanarReconstructPlanRun
 * stores.  |e| <= 65535.  The record of row (i, c) is four unsigned 64-bit integers:
 *     sum_sq = sum over t of e^2,  sum_abs = sum of |e|,  max_abs = max of |e| (0 for an empty row),  count = num_samples_i.
 * With M/S the error is taken on L / R, after the inverse transform, as the rows are.  The warm-up blocks of a segmented chain
 * and the trial search's measuring passes contribute nothing: every frame of a row counts exactly once.
 * 65535^2 * (2^32 - 1) < 2^64, so nothing wraps for any stream the format allows, and every field is non-negative as int64 for
 * rows below 2^31 frames.  The sums are integers, so they do not depend on the lane mapping, the segmentation's chains or the
 * order of anything: two runs give the same bits.
 *
 * The table is N * C records, contiguous, row (i, c) at index i * C + c: a torch int64 [N, C, 4] tensor on the device IS the table
 * (as an int64 [N, 2] tensor is the window table).
 *
 * AADHip_PlanarReconstructPlanRunStats is AADHip_PlanarReconstructPlanRun with the table as a further output:
 *   - images and rows are byte for byte what AADHip_PlanarReconstructPlanRun writes for the same inputs; no other element of
 *     `device_out` and nothing outside the N * C records is touched;
 *   - device_out may be NULL: statistics and images only, no rows are written;
 *   - every record is written by the run, whatever the table held before (a segmented plan's run clears it on the context's
 *     stream first: its chains add into it);
 *   - errors: those of AADHip_PlanarReconstructPlanRun (but for the null device_out), plus AAD_APIRESULT_INVALID_ARGUMENT for a
 *     null device_stats or one that is not 8-byte aligned while the plan has streams.  Plans of any other kind are refused; a plan
 *     without streams is OK and launches nothing;
 *   - AADHip_ContextSignalNextRun: the start event sits in front of the run's first device operation and the stop event behind
 *     its last.  An unsegmented plan's run is one kernel and both ride on it; a segmented plan's run is the clear and the kernel,
 *     the start event recorded in front of the clear and the stop event riding on the kernel. */
struct AADHipRowStats {
  uint64_t sum_sq;
  uint64_t sum_abs;
  uint64_t max_abs;
  uint64_t count;
};
AADApiResult AADHip_PlanarReconstructPlanRunStats(
    struct AADHipEncodePlan *plan, const void *device_samples, uint8_t *device_data,
    void *device_out,                     /* may be NULL here: statistics and images only */
    struct AADHipLaneState *device_state,
    struct AADHipRowStats *device_stats); /* N * C records, 8-byte aligned, every one written by the run */

/* ---- window reconstruct: device-drawn crops of a PCM corpus through the codec ------------------------------------------------- */

/* The write side of window decode: crops named by a window table IN DEVICE MEMORY (the host never reads it), read where they lie
 * in a corpus of planar int16 / float32 rows and run through the encoder - the planar reconstruct kernels, whose per-lane tables a
 * small kernel writes on the device from the windows.  No gather and no copy of the batch; a run is asynchronous on the context's
 * stream (one that needs larger tables than any run of the plan before it waits for the stream once, to replace them).
 *
 * Definition.  A plan holds an encode parameter, an optional segmentation, the input layout (sample type and channel_stride) and a
 * SOURCE TABLE of S streams, of which two fields are read: pcm_offset, the element that starts channel 0's row of source stream s
 * (channel c's row channel_stride * c elements further on), and num_samples = n_s, which may be 0.  A run takes the corpus, N
 * windows {stream, first_frame}, T = frames_per_window and its outputs.  For window w let
 *     len_w = 0                            if stream >= S or first_frame >= n_s
 *           = min(T, n_s - first_frame)    otherwise.
 * Huge or "negative" (wrapped int64) values are not an error: they give len_w = 0 and read nothing.
 *   len_w > 0:  the run writes exactly what AADHip_PlanarReconstructPlanRunStats writes for a plan with the same parameter,
 *     segmentation and input layout and fresh encoders in which stream w has num_samples = len_w, pcm_offset = the source's
 *     pcm_offset + first_frame, its image at data_offset = w * image_stride and its rows at
 *     w * output->stream_stride + c * output->channel_stride: the image bytes, the rows and the AADHipRowStats records w * C + c.
 *   len_w == 0: the image is the 31-byte file header with num_samples = 0 and no block; the four statistics fields are 0.
 *   Every row element t in [len_w, T) is written as zero: an [N, C, T] output is fully defined, as window decode's is.
 * Window w's length can be read from its records' `count`, or from bytes 14..17 of its image.
 * No byte outside the 31 + blocks(len_w) image bytes, the C rows of T elements and the C records of a window is touched.
 * Reads: no source element outside [first_frame, first_frame + len_w) of the window's C rows is read.  That is the rule of every
 * planar plan with ragged streams, and it holds because the planar kernels have no look-ahead past a stream's end: they load whole
 * 16-sample chunks only where all sixteen are the stream's, clamp every prefetch to the stream's last whole chunk, and read the
 * samples behind it one by one (the trial search looks one block BACK, inside the lane's own frames).  A crop next to another
 * stream's rows, or to the corpus's last element, is safe.
 *
 * Outputs.  Each of device_data, device_out and device_stats may be NULL, but not all three: images, rows, statistics or any
 * subset.  The encoders always write images; when they are not wanted they go to scratch that the context owns (grow-only, as the
 * trial scratch) and image_stride is ignored.  `output` may be NULL with device_out.
 * Not supported: carried state (crops start from fresh encoders) and interleaved sources of more than one channel (mono int16 IS
 * the interleaved layout, as elsewhere).
 *
 * The plan is an ordinary AADHipEncodePlan of a kind of its own: every other ...PlanRun refuses it and
 * AADHip_WindowReconstructPlanRun refuses every other plan (AAD_APIRESULT_INVALID_ARGUMENT); AADHip_EncodePlanDestroy destroys it
 * too.  One plan serves any N, any T and any output sample type; its device tables (one record per window and chain of the
 * uniform launch: N * ceil(blocks(T) / L) lanes, N unsegmented) grow when needed, on the context's stream.
 * Errors.  Create: those of AADHip_PlanarEncodePlanCreate for the parameter, layout and segmentation, AAD_APIRESULT_INVALID_ARGUMENT
 * for C > 1 with channel_stride below the longest n_s and for a source row end (pcm_offset + (C - 1) channel_stride + n_s) that
 * overflows 64 bits in elements or bytes.  Run: AAD_APIRESULT_INVALID_ARGUMENT for T == 0, all three outputs NULL while N > 0, with device_data
 * an image_stride < AADHip_CalculateEncodedSize(parameter, T) while N > 1 or images past 64 bits, with device_out a null or
 * refused `output` (sample type, reserved; rows of T elements that overlap or end past 64 bits, as the planar reconstruct plan's
 * rule with "longest" = T), more than UINT32_MAX lanes, device_out == device_samples, and, while N > 0, a null corpus, a null or
 * not 8-byte aligned window table or a not 8-byte aligned statistics table.  N == 0 is OK and launches nothing.
 * AADHip_ContextSignalNextRun: a run is several device operations - the resolve kernel (which also zeroes the row tails), the
 * clear of the statistics table (segmented, with device_stats), the encoder kernel.  The start event sits in front of the first
 * (it rides on the resolve kernel) and the stop event rides on the last, the encoder kernel.  A run that fails leaves the events
 * unsettled: refused arguments record neither, a HIP failure after the resolve launch may leave the start event recorded and the
 * stop event not - wait for neither after a failed run. */
AADApiResult AADHip_WindowReconstructPlanCreate(
    struct AADHipContext *context, const struct AADEncodeParameter *parameter,
    const struct AADHipPlanarLayout *input_layout,
    const struct AADHipSegmentation *segmentation, /* NULL: the serial (reference-exact) encode */
    uint32_t num_source_streams, const struct AADHipStreamDesc *source_streams,
    struct AADHipEncodePlan **plan);
void AADHip_WindowReconstructPlanDestroy(struct AADHipEncodePlan *plan);
AADApiResult AADHip_WindowReconstructPlanRun(
    struct AADHipEncodePlan *plan, const void *device_samples,
    uint64_t num_windows, const struct AADHipWindow *device_windows, /* device memory, 8-byte aligned: a torch int64 [N, 2] tensor */
    uint32_t frames_per_window,
    uint64_t image_stride, uint8_t *device_data, /* NULL: the images go to the context's scratch */
    const struct AADHipPlanarOutput *output, void *device_out, /* NULL (both may be): no rows */
    struct AADHipRowStats *device_stats);        /* NULL: no statistics; else N * C records, 8-byte aligned */

/* ---- host-memory convenience (stage -> run -> copy back, synchronous) ---------------------- */

/* pcm[i]: num_samples[i] interleaved frames; data[i]: data_capacity[i] bytes; output_size[i]
 * (may be NULL) receives the image size.  state: NULL for fresh encoders, else a host array of
 * num_streams * num_channels records, read before and written after the run. */
AADApiResult AADHip_EncodeBatch(
    struct AADHipContext *context, const struct AADEncodeParameter *parameter,
    uint32_t num_streams, const int16_t *const *pcm, const uint32_t *num_samples,
    uint8_t *const *data, const uint64_t *data_capacity, uint64_t *output_size,
    struct AADHipLaneState *state);

/* AADHip_EncodeBatch for a segmented encode: for the same PCM, parameter and segmentation, exactly the bytes of
 * AADHip_SegmentedEncodePlanCreate + AADHip_EncodePlanRun on device-resident copies (see above the struct AADHipSegmentation).
 * No state argument: a segmented encode starts from fresh encoders.  As in AADHip_ReconstructBatch, the compute runs over a WAVE
 * resident on the device: every chain of it, each with its warm-up frames, in one launch.  The PCM goes up and the images come
 * down through the context's pinned blocks in chunks.  A batch beyond three quarters of the device's free memory runs as several
 * waves of consecutive chains.  Results do not depend on any of it.
 * Errors are those of AADHip_EncodeBatch, plus AAD_APIRESULT_INVALID_ARGUMENT for a null `segmentation`, segment_blocks == 0 and
 * more than UINT32_MAX chains in the batch. */
AADApiResult AADHip_SegmentedEncodeBatch(
    struct AADHipContext *context, const struct AADEncodeParameter *parameter,
    const struct AADHipSegmentation *segmentation,
    uint32_t num_streams, const int16_t *const *pcm, const uint32_t *num_samples,
    uint8_t *const *data, const uint64_t *data_capacity, uint64_t *output_size);

/* data[i]/data_size[i]: .aad images (all of one format); pcm[i] must hold
 * pcm_capacity_frames[i] >= header.num_samples frames.  decoded_frames[i] (may be NULL) receives
 * the frames written: header.num_samples, or fewer when the image ends early - the reference's
 * block walk stops when the bytes run out (src/aad_decoder.c:514) and so does this. */
AADApiResult AADHip_DecodeBatch(
    struct AADHipContext *context, uint32_t num_streams,
    const uint8_t *const *data, const uint64_t *data_size,
    int16_t *const *pcm, const uint32_t *pcm_capacity_frames, uint32_t *decoded_frames);

/* ---- reconstruction modes: encode -> decode -> residual / statistics, all on the device ------ */

/* What the reference CLI's -r / -g / -c modes compute (src/main.c:275-503) for MANY inputs
 * without the encoded images or the reconstructed PCM ever leaving HBM.  Per stream:
 *   images  = AADEncoder_EncodeWhole(pcm)          (src/main.c:319-325)
 *   out     = AADDecoder_DecodeWhole(images)       (src/main.c:328-332)        -> `aad -r`
 *   out     = int16 wrap of pcm - out              (src/main.c:419-423)        -> `aad -g`
 *   stats   = RMSE / MSD / MaxAE as `aad -c` prints them (src/main.c:476-497)  -> `aad -c`
 */
enum AADHipReconstructOutput {
  AAD_HIP_RECONSTRUCT_DECODED = 0, /* out holds the reconstructed PCM */
  AAD_HIP_RECONSTRUCT_RESIDUAL = 1 /* out holds original minus reconstructed */
};

/* the three numbers of `aad -c`'s "RMSE:%f MSD:%f MaxAE:%f" line, per stream */
struct AADHipErrorStats {
  double rms_error;
  double mean_abs_error;
  double max_abs_error;
};

struct AADHipReconstructPlan;

/* `streams` as for AADHip_EncodePlanCreate: pcm_offset addresses BOTH the input and the output
 * PCM buffer, data_offset / data_size the scratch buffer that receives the .aad images. */
AADApiResult AADHip_ReconstructPlanCreate(
    struct AADHipContext *context, const struct AADEncodeParameter *parameter,
    uint32_t num_streams, const struct AADHipStreamDesc *streams,
    struct AADHipReconstructPlan **plan);
void AADHip_ReconstructPlanDestroy(struct AADHipReconstructPlan *plan);

/* device_stats: NULL, or num_streams records, the same doubles whichever output_kind (AAD_HIP_OPTION_COMPARE_ORDER holds for
 * both).  Fresh encoders (as the CLI creates per file). */
AADApiResult AADHip_ReconstructPlanRun(
    struct AADHipReconstructPlan *plan, const int16_t *device_pcm, uint8_t *device_data,
    int16_t *device_out, int32_t output_kind, struct AADHipErrorStats *device_stats);

/* host-memory form.  out_pcm: NULL (statistics only - nothing but 24 bytes per stream comes
 * back over PCIe) or per-stream buffers of num_samples[i] frames; stats: NULL or num_streams.
 * Any batch size: the compute runs over a WAVE of whole streams resident on the device (one ReconstructPlanRun: the encoders'
 * block chains side by side, the statistics summed per stream as the plan form does), the PCM goes up and the output comes down
 * through the context's pinned blocks in chunks of the tile budget (AAD_HIP_OPTION_TILE_KBYTES), and a batch beyond three
 * quarters of the device's free memory is run as several waves of consecutive streams.  Results do not depend on any of it. */
AADApiResult AADHip_ReconstructBatch(
    struct AADHipContext *context, const struct AADEncodeParameter *parameter,
    uint32_t num_streams, const int16_t *const *pcm, const uint32_t *num_samples,
    int32_t output_kind, int16_t *const *out_pcm, struct AADHipErrorStats *stats);

/* The reconstruction modes over the images of a segmented encode (AADHip_SegmentedEncodePlanCreate): the images are the segmented
 * ones, the statistics keep their meaning - the decoded segmented image against the original, with the same tie rule and
 * AAD_HIP_OPTION_COMPARE_ORDER.  The plan is an ordinary one: AADHip_ReconstructPlanRun and AADHip_ReconstructPlanDestroy work on
 * it.  The batch form takes the waves and chunked staging of AADHip_ReconstructBatch.  Errors are those of the unsegmented forms,
 * plus AAD_APIRESULT_INVALID_ARGUMENT for a null `segmentation`, segment_blocks == 0 and more than UINT32_MAX chains. */
AADApiResult AADHip_SegmentedReconstructPlanCreate(
    struct AADHipContext *context, const struct AADEncodeParameter *parameter,
    const struct AADHipSegmentation *segmentation,
    uint32_t num_streams, const struct AADHipStreamDesc *streams,
    struct AADHipReconstructPlan **plan);
AADApiResult AADHip_SegmentedReconstructBatch(
    struct AADHipContext *context, const struct AADEncodeParameter *parameter,
    const struct AADHipSegmentation *segmentation,
    uint32_t num_streams, const int16_t *const *pcm, const uint32_t *num_samples,
    int32_t output_kind, int16_t *const *out_pcm, struct AADHipErrorStats *stats);

#ifdef __cplusplus
}
#endif

#endif /* AAD_HIP_H_INCLUDED */
