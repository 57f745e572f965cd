/*
 * smpc_debug.h — developer entry points of libsmpc.so.
 *
 * These are aids for the tests, the tools and the benchmark: they read back
 * what a tick left behind or run one piece of the library on its own.  They
 * are NOT part of the ABI of include/smpc.h: no stability promise, no ABI
 * version, and any of them may change or go with the code it looks into.
 * They are declared here so that the compiler holds each definition to one
 * signature and the ctypes mirror (_abi.DEBUG_PROTOTYPES) has one text to
 * follow.  Return values are SMPC_OK or SMPC_ERR_* unless stated.
 */
#ifndef SMPC_DEBUG_H_
#define SMPC_DEBUG_H_

#include "smpc.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the scoring-pass instance the calling thread launched last, spelled as a
 * kernel trace spells it; "" before the first launch */
const char* smpc_debug_last_pass_kernel(void);

/* 1: this ctx hands its per-tick inputs over by CPU stores through the PCIe
 * BAR; 0: by a copy on the stream or inside the kernel arguments */
int smpc_debug_bar_tick(const smpc_ctx* ctx);

/* SMPC_FLAG_PROFILE: GPU time of the last acceleration-limit launch */
int smpc_debug_limit_ms(smpc_ctx* ctx, float* ms);

/* SMPC_FLAG_PROFILE: GPU time of the last moving-obstacle launch */
int smpc_debug_moving_ms(smpc_ctx* ctx, float* ms);

/* launches of the grouped moving-obstacle kernels (one per form and round,
 * however many members ride) and uploads of the group's table buffer
 * (smpc_group_set_moving_obstacles) so far; either pointer may be NULL */
int smpc_debug_group_moving_launches(const smpc_group* group, uint64_t* grouped_launches, uint64_t* table_uploads);

/* on != 0: the group's riding members with moving obstacles keep one
 * moving-obstacle launch each, in front of the hand-over, instead of the
 * grouped launch (the route the grouped one replaced; same results) — for
 * measuring the two routes in one process (SMPC_FLEET_AVOID=per_member) */
int smpc_debug_group_moving_per_member(smpc_group* group, int on);

/* SMPC_FLAG_PROFILE: GPU time of the last breakdown's scoring pass and of
 * its reduction */
int smpc_debug_stats_ms(const smpc_ctx* ctx, float* pass_ms, float* reduce_ms);

/* the float F = index + fraction the last tick's scoring pass reported, as
 * kept for the next prediction */
int smpc_debug_furthest_f(const smpc_ctx* ctx, float* F);

/* stamps of the last launch's grid tail: out[8][16] */
int smpc_debug_tail_timeline(smpc_ctx* ctx, unsigned long long* out);

/* stage durations of the last lane-pass launch: out[7][3] = min, median, max,
 * then out[21..28] per wave of the block; n_blocks may be NULL */
int smpc_debug_lane_timeline(smpc_ctx* ctx, double* out, uint32_t* n_blocks);

/* SMPC_LANE_TIMELINE=1: groups of the lane pass that took the furthest-point
 * scan since the last call (cleared by it), and the groups of one launch;
 * groups_per_launch may be NULL */
int smpc_debug_lane_scan_count(smpc_ctx* ctx, unsigned long long* scanned, uint32_t* groups_per_launch);

/* host only: the prune table a tick would write for this plan and first
 * index; out: SMPC_PRUNE_FLOATS floats */
int smpc_debug_prune_table(const float* px, const float* py, uint32_t P, uint32_t k0, int on, float* out);

/* host only: the LDS carve-up a scoring pass is launched with (kind 0: wave,
 * 1: lane, 2: split pass); out: the 16 words of the layout */
int smpc_debug_lds_layout(int kind, uint32_t window_bytes, uint32_t P, uint32_t T, uint32_t arg, uint32_t* out);

/* the split pass's N x N transpose-reduce per group of N lanes:
 * v [64 lanes][n] -> out [64], n = 16 or 32 */
int smpc_selftest_row_reduce(smpc_ctx* ctx, const float* v, uint32_t n, float* out);

#ifdef __cplusplus
}
#endif

#endif /* SMPC_DEBUG_H_ */
