/*
 * ref_state.c - test infrastructure: the REFERENCE encoder with a setter and a getter for the carried predictor state of a
 * handle (struct AADEncodeProcessor: weight[4], history[4], table.stepsize_index, quantize_error), which its public API keeps
 * private.  Written here, not copied: this file stands in for the reference's encoder source in oracle/_ref/libaadref_state.so
 * - it includes that source by name where it lies (-I$(REF)/src), so the two functions below see the struct - next to the
 * reference's decoder, tables and ref_batch.c.  oracle/_ref/libaadref.so is not touched.
 *
 * Used by tests/golden/make_crafted_state_golden.py and tests/test_crafted_state.py to start the reference from crafted records
 * (tests/crafted_state.py) and to read the complete record back after a call.
 *
 * AADEncoder_SetEncodeParameter resets every channel's step index (reference src/aad_encoder.c:797-799), so a record is set
 * AFTER it.  The reference keeps the index in an int16 and asserts 0 .. 4080 << 4 on it: callers pass an index inside that range.
 */
#include <stdint.h>

#include "aad_encoder.c"

int aadref_set_lane(struct AADEncoder *encoder, uint32_t ch, const int32_t *w, int32_t idx, int32_t qerr)
{
  uint32_t k;
  if (encoder == NULL || w == NULL || ch >= AAD_MAX_NUM_CHANNELS) return -1;
  for (k = 0; k < AAD_FILTER_ORDER; k++) encoder->processor[ch].weight[k] = w[k];
  encoder->processor[ch].table.stepsize_index = (int16_t)idx;
  encoder->processor[ch].quantize_error = qerr;
  return 0;
}

int aadref_get_lane(const struct AADEncoder *encoder, uint32_t ch, int32_t *w, int32_t *h, int32_t *idx, int32_t *qerr)
{
  uint32_t k;
  if (encoder == NULL || w == NULL || h == NULL || idx == NULL || qerr == NULL || ch >= AAD_MAX_NUM_CHANNELS) return -1;
  for (k = 0; k < AAD_FILTER_ORDER; k++) {
    w[k] = encoder->processor[ch].weight[k];
    h[k] = encoder->processor[ch].history[k];
  }
  *idx = encoder->processor[ch].table.stepsize_index;
  *qerr = encoder->processor[ch].quantize_error;
  return 0;
}
