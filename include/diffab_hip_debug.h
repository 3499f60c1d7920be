/* diffab_hip_debug.h - test hooks of libdiffab_hip.so that are NOT part of the public C ABI (include/diffab_hip.h): exported so that a
 * test can reach a piece of internal logic, free to change with it. */
#ifndef DIFFAB_HIP_DEBUG_H
#define DIFFAB_HIP_DEBUG_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The start classes of the module launch's work-groups from a row plan (diffab_debug_row_plan's [B][2 + K / 16] ints): out[b] in
 * 0 .. classes - 1, B bytes.  on_device = 0: plan and out are HOST memory, the ranking function runs on the host (no device needed);
 * on_device != 0: both are device memory and the sampler's own kernel is enqueued on `stream`.  1 <= classes <= 256, K a multiple
 * of 16 in 16 .. 1024. */
int diffab_debug_start_classes(const int32_t* plan, int32_t B, int32_t K, int32_t classes, uint8_t* out, int32_t on_device, void* stream);

#ifdef __cplusplus
}
#endif
#endif
