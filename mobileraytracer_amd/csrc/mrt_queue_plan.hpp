// mrt_queue_plan.hpp - sizes of the wavefront queues (host only, no HIP): the first allocation, the
// plan after an overflowed pass from what that pass asked for, and the worst-case plan.
// DESIGN.md section 2, "Queue plans"; exported as mrt_plan_queues (include/mobilert_amd.h).
#pragma once

#include <cstdint>
#include <string>

#include "mobilert_amd.h"

namespace mrt {

constexpr int kPlanLevels = MRT_QUEUE_LEVELS;
constexpr int kPlanSegments = 8;        // mrt_queue_plan_request.segments <= 0
constexpr int kPlanGrowthPct = 200;     // ... growthPct <= 0 (tuning key 38)
constexpr int kPlanSlack = 3 * 4 * 256; // ... slack < 0 (tuning key 39)
constexpr int64_t kPlanPathBudget = int64_t{1} << 24;  // ... pathBudget <= 0
// counters and Level::cap are int: every capacity, and with it every segment demand a plan was
// sized for, stays below this
constexpr int64_t kPlanCapLimit = int64_t{1} << 30;
// demand-driven plans of one frame (or progressive sample) before the worst-case plan
constexpr int kPlanDemandRetries = 3;

// Bytes of one ray slot (rO, rD, tree, hit, vtx, res; kd and last when textured) and of one shadow
// slot (sO, sD, sC), as allocQueues allocates them.
int64_t planRaySlotBytes(bool textured);
int64_t planShadowSlotBytes();

// The plan for `q`.  false with *err set: a malformed request, or no chunk of at least one pixel
// slot fits the byte budget (for the worst-case plan: "one pixel's worst-case ray tree ...").
bool planQueues(const mrt_queue_plan_request& q, mrt_queue_plan* out, std::string* err);

// The per-lane walks' spill stacks, which the plans above do not count: two areas (the closest-hit
// and the any-hit walk's, which run together) of `threads` x `gdepth` entries of 8 bytes, thread k's
// at the 32-bit offset k * gdepth * 2 (in 4-byte words: makeRefStack).  Returns their bytes, or -1
// with *err set where the last thread's area would end past 2^31 words or the two areas exceed
// `availBytes` (what the device has left beside the queues; <= 0: not checked).
int64_t planSpillBytes(int64_t threads, int64_t gdepth, int64_t availBytes, std::string* err);

}  // namespace mrt
