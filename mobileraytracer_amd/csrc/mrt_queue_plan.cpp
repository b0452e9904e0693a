// mrt_queue_plan.cpp - the queue planner (mrt_queue_plan.hpp).  Pure host code.
#include "mrt_queue_plan.hpp"

#include <algorithm>
#include <cmath>

namespace mrt {

namespace {

struct Caps {
    int64_t seg[kPlanLevels] = {};
    int64_t shadow[kPlanLevels] = {};
};

// the request with its defaults filled in
struct Params {
    int levels, B, spp, spl, S, growthPct, slack, shadowSlack;
    bool textured;
    int64_t nSlots, pathBudget, byteBudget;
};

constexpr int64_t kHuge = int64_t{1} << 40;  // estimates saturate here (far above kPlanCapLimit)

int64_t ceilDiv(int64_t a, int64_t b) { return (a + b - 1) / b; }
int64_t sat(int64_t v) { return std::min(v, kHuge); }
int64_t satMul(int64_t a, int64_t b) { return (a != 0 && b > kHuge / a) ? kHuge : sat(a * b); }
// a * num / den rounded up, saturating (a, num < 2^40, den >= 1)
int64_t scaleUp(int64_t a, int64_t num, int64_t den) {
    const long double v = std::ceil(static_cast<long double>(a) * static_cast<long double>(num) / static_cast<long double>(den));
    return v >= static_cast<long double>(kHuge) ? kHuge : static_cast<int64_t>(v);
}
// 1.25 x the demand, plus the fixed slack
int64_t padded(int64_t demand, int64_t slack) { return sat(ceilDiv(satMul(demand, 5), 4) + slack); }

// The first allocation: a deeper level holds growthPct of level 1, an eighth of it (x 1.25) plus
// the slack per segment - the sizes every renderer starts with.
Caps firstCaps(const Params& p, int64_t chunk) {
    Caps c;
    const int64_t n1 = chunk * p.spp;
    const int64_t capN = n1 * p.growthPct / 100;
    for (int l = 1; l <= p.levels; ++l) {
        int64_t seg, sh;
        if (p.S == 1) {
            seg = l == 1 ? n1 : capN;
            sh = seg * p.spl;
        } else if (l == 1) {
            seg = ceilDiv(n1, p.S);
            sh = (n1 * p.spl * 5 / 4 + p.S - 1) / p.S + p.shadowSlack;
        } else {
            seg = (capN * 5 / 4 + p.S - 1) / p.S + p.slack;
            sh = (capN * p.spl * 5 / 4 + p.S - 1) / p.S + p.shadowSlack;
        }
        c.seg[l - 1] = seg;
        c.shadow[l - 1] = sh;
    }
    return c;
}

// Most parents of one queue segment among `count` vertices of a level: the shading hands its
// vertices to the segments in blocks of 256 (k_shade) or 64 (the fused level 1), round robin.
int64_t segParents(int64_t count, int S) {
    const int64_t by256 = 256 * ceilDiv(ceilDiv(count, 256), S);
    const int64_t by64 = 64 * ceilDiv(ceilDiv(count, 64), S);
    return std::min(count, std::max(by256, by64));
}

// The worst case: every hit spawns B children and spl shadow rays.  Level l then has n1 * B^(l-1)
// rays at most; a segment of level l + 1 gets the children of at most segParents of them.
Caps worstCaps(const Params& p, int64_t chunk) {
    Caps c;
    const int64_t n1 = chunk * p.spp;
    int64_t count = n1;  // most rays of level l
    for (int l = 1; l <= p.levels; ++l) {
        const int64_t parents = p.S == 1 ? count : segParents(count, p.S);
        if (l == 1) c.seg[0] = ceilDiv(n1, p.S);  // (dense: denseCounts)
        c.shadow[l - 1] = satMul(parents, p.spl);
        if (l < p.levels) c.seg[l] = satMul(parents, p.B);
        count = satMul(count, p.B);
    }
    return c;
}

// After an overflowed pass.  Its per-segment demand is exact up to the first overflowed level f
// (the parents of those levels were all there) and a lower bound below it.  Exact levels: the
// largest segment's demand, scaled to this chunk, x 1.25 plus the slack.  Deeper levels: the last
// exact level extrapolated with the ratio of the last two exact levels, clamped to [1, B], and
// never less than the lower bound.  No level's capacity per path shrinks.
Caps demandCaps(const Params& p, const mrt_queue_plan_request& q, int64_t chunk) {
    Caps c;
    const int64_t n1 = chunk * p.spp;
    // the paths a chunk of this size runs per pass, as the recorded pass did (progressive: 1 sample)
    const int64_t num = std::max<int64_t>(1, scaleUp(chunk, q.demandPaths, q.demandChunkSlots));
    const int64_t den = q.demandPaths;
    int f = 1;
    while (f < p.levels && ((q.overflowMask >> f) & 1) == 0) ++f;
    const bool havePrev = q.prevChunkSlots > 0;
    // level f's own ray queue dropped rays (then its shadow rays and level f + 1 are lower bounds too)
    const bool raysDropped = !havePrev || q.segDemand[f - 1] > q.prevSegCap[f - 1];
    const int exactRay = std::min(p.levels, raysDropped ? f : f + 1);
    const int exactShadow = raysDropped ? f - 1 : f;
    int64_t D[kPlanLevels], Sh[kPlanLevels], est[kPlanLevels];
    for (int l = 1; l <= p.levels; ++l) {
        D[l - 1] = scaleUp(std::max<int64_t>(0, q.segDemand[l - 1]), num, den);
        Sh[l - 1] = scaleUp(std::max<int64_t>(0, q.shadowSegDemand[l - 1]), num, den);
    }
    double g = static_cast<double>(p.B);
    if (exactRay >= 2 && D[exactRay - 2] > 0)
        g = std::min(static_cast<double>(p.B),
                     std::max(1.0, static_cast<double>(D[exactRay - 1]) / static_cast<double>(D[exactRay - 2])));
    // shadow rays per ray: the most any exact level showed, at most spl
    double s = -1.0;
    for (int l = 1; l <= exactShadow; ++l)
        if (D[l - 1] > 0) s = std::max(s, static_cast<double>(Sh[l - 1]) / static_cast<double>(D[l - 1]));
    s = s < 0.0 ? static_cast<double>(p.spl) : std::min(s, static_cast<double>(p.spl));
    for (int l = 1; l <= p.levels; ++l) {
        if (l <= exactRay) {
            est[l - 1] = D[l - 1];
        } else {
            const double e = std::ceil(static_cast<double>(est[l - 2]) * g);
            est[l - 1] = std::max(D[l - 1], e >= static_cast<double>(kHuge) ? kHuge : static_cast<int64_t>(e));
        }
        int64_t sh = Sh[l - 1];
        if (l > exactShadow) {
            const double e = std::ceil(static_cast<double>(est[l - 1]) * s);
            sh = std::max(sh, e >= static_cast<double>(kHuge) ? kHuge : static_cast<int64_t>(e));
        }
        c.seg[l - 1] = l == 1 ? ceilDiv(n1, p.S) : padded(est[l - 1], p.slack);
        c.shadow[l - 1] = padded(sh, p.shadowSlack);
        if (havePrev) {
            // (per path: what the previous plan held beyond the fixed slack, scaled to this chunk)
            const int64_t n1Prev = q.prevChunkSlots * p.spp;
            const int64_t seg = std::max<int64_t>(0, q.prevSegCap[l - 1] - p.slack);
            const int64_t sh = std::max<int64_t>(0, q.prevShadowSegCap[l - 1] - p.shadowSlack);
            if (l > 1) c.seg[l - 1] = std::max(c.seg[l - 1], sat(scaleUp(seg, n1, n1Prev) + p.slack));
            c.shadow[l - 1] = std::max(c.shadow[l - 1], sat(scaleUp(sh, n1, n1Prev) + p.shadowSlack));
        }
    }
    return c;
}

}  // namespace

int64_t planRaySlotBytes(bool textured) {
    // rO, rD: float4; tree: uint32; hit: float4; vtx: int4; res: float4; kd, last: float4
    return 16 + 16 + 4 + 16 + 16 + 16 + (textured ? 32 : 0);
}

int64_t planShadowSlotBytes() { return 3 * 16; }  // sO, sD, sC: float4

int64_t planSpillBytes(int64_t threads, int64_t gdepth, int64_t availBytes, std::string* err) {
    if (threads < 1 || gdepth < 1 || threads > (int64_t{1} << 31) || gdepth > (int64_t{1} << 24)) {
        *err = "spill stacks: threads 1 .. 2^31, depth 1 .. 2^24";
        return -1;
    }
    // the end of the last thread's area in words: every index gofs + sp - depth stays an int
    if (threads * gdepth * 2 > (int64_t{1} << 31) - 1) {
        *err = "the scene's tree is too deep for the walks' spill stacks: " + std::to_string(threads) + " threads x " +
               std::to_string(gdepth) + " entries pass the 32-bit offsets";
        return -1;
    }
    const int64_t bytes = 2 * threads * gdepth * 8;
    if (availBytes > 0 && bytes > availBytes) {
        *err = "the scene's tree is too deep for the device memory: the walks' spill stacks need " +
               std::to_string(bytes) + " bytes beside the queues, " + std::to_string(availBytes) + " are left";
        return -1;
    }
    return bytes;
}

bool planQueues(const mrt_queue_plan_request& q, mrt_queue_plan* out, std::string* err) {
    Params p{};
    p.levels = q.levels;
    p.B = q.branching;
    p.spp = q.samplesPixel;
    p.spl = q.samplesLight;
    p.S = q.segments > 0 ? q.segments : kPlanSegments;
    p.growthPct = q.growthPct > 0 ? q.growthPct : kPlanGrowthPct;
    p.slack = q.slack >= 0 ? q.slack : kPlanSlack;
    p.shadowSlack = p.spl * (p.slack / 3);  // (3072 -> 1024 per light sample)
    p.textured = q.textured != 0;
    p.nSlots = q.pixelSlots;
    p.pathBudget = q.pathBudget > 0 ? q.pathBudget : kPlanPathBudget;
    p.byteBudget = q.byteBudget;
    if (p.levels < 1 || p.levels > kPlanLevels || p.B < 1 || p.B > 4 || p.spp < 1 || p.spl < 1 || p.S > 64 ||
        p.nSlots < 1 || p.nSlots > (int64_t{1} << 31) || p.pathBudget > (int64_t{1} << 31) || p.spp > (1 << 20) || p.spl > (1 << 20) ||
        p.growthPct > 100000 || p.slack > (1 << 24)) {
        *err = "queue plan: levels 1-16, branching 1-4, samples and pixel slots >= 1, path budget <= 2^31";
        return false;
    }
    const bool worst = q.worstCase != 0;
    const bool demand = !worst && q.hasDemand != 0;
    if (demand) {
        bool bad = q.demandChunkSlots < 1 || q.demandPaths < 1 || q.demandChunkSlots > (int64_t{1} << 31) ||
                   q.demandPaths > kHuge || (q.overflowMask >> 1) == 0 || q.prevChunkSlots > (int64_t{1} << 31);
        for (int l = 0; l < p.levels; ++l)
            bad = bad || q.segDemand[l] > kHuge || q.shadowSegDemand[l] > kHuge || q.prevSegCap[l] > kHuge ||
                  q.prevShadowSegCap[l] > kHuge || q.prevSegCap[l] < 0 || q.prevShadowSegCap[l] < 0;
        if (bad) {
            *err = "queue plan: the demand record needs the pass's chunk, its paths and an overflowed level";
            return false;
        }
    }
    const int64_t rayBytes = planRaySlotBytes(p.textured), shadowBytes = planShadowSlotBytes();
    Caps caps;
    int64_t bytes = 0;
    // whether a chunk of this many slots fits the byte budget and the int range (fills caps, bytes)
    auto fits = [&](int64_t chunk) {
        caps = worst ? worstCaps(p, chunk) : demand ? demandCaps(p, q, chunk) : firstCaps(p, chunk);
        bytes = 0;
        bool ok = true;
        for (int l = 0; l < p.levels; ++l) {
            const int64_t cap = satMul(caps.seg[l], p.S), shadowCap = satMul(caps.shadow[l], p.S);
            ok = ok && cap < kPlanCapLimit && shadowCap < kPlanCapLimit;
            bytes = sat(bytes + sat(satMul(cap, rayBytes) + satMul(shadowCap, shadowBytes)));
        }
        return ok && (p.byteBudget <= 0 || bytes <= p.byteBudget);
    };
    // every slot of the shard in one chunk, within the path budget ...
    int64_t chunk = std::max<int64_t>(1, std::min(p.nSlots, p.pathBudget / p.spp));
    if (!fits(chunk)) {
        // ... else the largest chunk that fits (the capacities grow with the chunk)
        if (!fits(1)) {
            *err = worst ? "one pixel's worst-case ray tree does not fit the queue byte budget"
                         : "queue plan: no chunk fits the queue byte budget";
            return false;
        }
        int64_t lo = 1, hi = chunk;  // lo fits, hi does not
        while (hi - lo > 1) {
            const int64_t mid = lo + (hi - lo) / 2;
            if (fits(mid)) {
                lo = mid;
            } else {
                hi = mid;
            }
        }
        chunk = lo;
        fits(chunk);
    }
    *out = mrt_queue_plan{};
    out->chunkSlots = chunk;
    for (int l = 0; l < p.levels; ++l) {
        out->segCap[l] = caps.seg[l];
        out->shadowSegCap[l] = caps.shadow[l];
    }
    out->bytes = bytes;
    out->worstCase = worst ? 1 : 0;
    return true;
}

}  // namespace mrt
