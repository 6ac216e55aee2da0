// The LDS schedule of the 8-wave ("wide") posterior kernel
// (post_partials_wide_kernel, post.hip), written once for the kernel and for
// the host (bo_post_wide_schedule, which the tests walk).
//
// A k-step is four k-slices; a *unit* is half a step, unit u = 2 step + h
// holding slices 2 h and 2 h + 1.  The U ring's stages hold kSS consecutive
// steps of the walk (a super-step: kNU = 2 kSS units), so the workgroup meets
// at a barrier once per super-step; one workgroup per CU has the LDS for it
// (kStages x kSS x 16 rows x 144 doubles).
//
// A segment of nsteps k-steps is nss = ceil(nsteps / kSS) super-steps and
// nss + 1 barrier intervals: interval j lies between barrier j and barrier
// j + 1 (barrier 0 closes the prologue, which writes super-step 0 into stage
// 0).  In interval j a wave multiplies the kNU units from kNU j - lag on, lag
// = 0 for the early half of the workgroup (waves 0-3) and kLag for the late
// half (waves 4-7, BO_POSTW_STAGGER): the late half trails by kLag units, so
// the two waves of a SIMD reach their LDS reads, their U store and the barrier
// from different places.  Both halves store their share of super-step j + 1 in
// interval j: the early half at its end, in front of the barrier, the late
// half after its first kNU / 2 units, its drain under the units that follow.
// The late half reads the first slice of interval j + 1 at the end of interval
// j (its stage is complete by then); the early half's is being written in
// interval j, so it reads it behind the barrier.  The last interval holds only
// the late half's trailing units.  The shipped build has no stagger (kLag =
// 0: it measured slower): all eight waves run the
// early half's program and the last interval is empty.
//
// Stage safety: interval j writes stage (j + 1) % kStages and reads the stages
// of super-steps j - 1 and j; a barrier separates intervals, so three stages
// would do, and kStages = 4 makes the wrap a mask.
#pragma once

#ifndef BO_POSTW_STAGGER
#define BO_POSTW_STAGGER 0  // 1: waves 4-7 trail by BO_POSTW_LAG units (A/B: it lost)
#endif
#ifndef BO_POSTW_SS
#define BO_POSTW_SS 2  // k-steps per LDS stage and barrier (1 or 2)
#endif
#ifndef BO_POSTW_LAG
#define BO_POSTW_LAG 1  // units the late half trails by (1 .. 2 BO_POSTW_SS)
#endif

#if defined(__HIPCC__) || defined(__CUDACC__)
#define BO_POSTW_HD __host__ __device__
#else
#define BO_POSTW_HD
#endif

namespace postw {

constexpr int kStages = 4;
constexpr int kSlices = 4;  // k-slices (MFMA k = 4) per 16-row k-step
constexpr int kSS = BO_POSTW_SS;
constexpr int kNU = 2 * kSS;  // units per interval
constexpr int kLag = BO_POSTW_STAGGER ? BO_POSTW_LAG : 0;
static_assert(kSS >= 1 && kLag >= 0 && kLag <= kNU, "the late half reads at most one stage back");

BO_POSTW_HD constexpr int supersteps(int nsteps) { return (nsteps + kSS - 1) / kSS; }
// barriers a wave executes in one segment: the same expression for both halves
BO_POSTW_HD constexpr int barriers(int nsteps) { return supersteps(nsteps) + 2; }
BO_POSTW_HD constexpr int intervals(int nsteps) { return supersteps(nsteps) + 1; }
BO_POSTW_HD constexpr int lag_of(bool late) { return late ? kLag : 0; }

// First training row of walk step `step` (kbeg = 0): ascending, or (rev, the
// short partner tile) descending from the last step; steps past the last one
// repeat it (the duplicate rows of a ragged last super-step).
BO_POSTW_HD constexpr int walk_k0(int step, int nsteps, bool rev, int pk) {
  const int s = step < nsteps ? step : nsteps - 1;
  return (rev ? nsteps - 1 - s : s) * pk;
}

// Unit u: its step, its first slice, the stage and the stage row of its step.
BO_POSTW_HD constexpr bool unit_valid(int u, int nsteps) { return u >= 0 && u < 2 * nsteps; }
BO_POSTW_HD constexpr int unit_step(int u) { return u >> 1; }
BO_POSTW_HD constexpr int unit_slice0(int u) { return (u & 1) * (kSlices / 2); }
BO_POSTW_HD constexpr int stage_of_step(int step) { return (step / kSS) & (kStages - 1); }
BO_POSTW_HD constexpr int stage_row_of_step(int step, int pk) { return (step % kSS) * pk; }

// The k-th unit (0 <= k < kNU) of a half in interval j.
BO_POSTW_HD constexpr int unit_at(int j, int k, bool late) { return kNU * j - lag_of(late) + k; }
// The super-step interval j stores (into stage (j + 1) % kStages), -1: none;
// the late half stores after unit kNU / 2 - 1, the early half after the last.
BO_POSTW_HD constexpr int store_superstep(int j, int nsteps) {
  return j < supersteps(nsteps) ? j + 1 : -1;
}
BO_POSTW_HD constexpr int store_after_unit(bool late) { return late ? kNU / 2 - 1 : kNU - 1; }
// Whether a half reads the first slice of interval j + 1 at the end of
// interval j (else behind the barrier): its stage must be complete already.
BO_POSTW_HD constexpr bool prefetches(bool late) { return lag_of(late) > 0; }

}  // namespace postw
