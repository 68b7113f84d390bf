/*
 * har_switches.h -- the run-time switches (environment variables, docs/switches.md) of the C ABI's host code, parsed ONCE into one table.
 *
 * HIP-free.  switches() parses from getenv on its first call and never again, so every reader sees the same value whatever the call order;
 * parse_switches takes the getter as an argument (tests/test_switches_cpu.py).  HAR_TOP_SEED is NOT here: it is read whenever an integrator
 * is created or a scene is lowered (one process can hold both kinds).  The builder, the scene host, the kernels' launch wrappers and the
 * multi-GPU driver read their own variables.
 */
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstdlib>

namespace har {

constexpr int SWITCH_SHARDS = 8;        /* HAR_SHARDS (har_kernels.h; har_capi.hip asserts the two agree): HAR_TRACE_GRID is a multiple of it */

struct Switches {
    int      debug_guard = 0;           /* HAR_DEBUG_GUARD = 1 | 2: every device buffer between unmapped ranges, flush against the end / the start of its pages */
    bool     debug_sync = false;        /* HAR_DEBUG_SYNC (presence): name every launch class on stderr and wait for it */
    bool     texel_queues = true;       /* HAR_TEXEL_QUEUES=0: texel gradients by direct atomics */
    size_t   tq_lds = 0;                /* HAR_TQ_LDS: LDS bytes of a texel band, 0 = automatic */
    uint32_t tq_bpq = 0;                /* HAR_TQ_BPQ: blocks per texel queue, 0 = automatic */
    int      overlap = -1;              /* HAR_OVERLAP: -1 by job size, 0 off, else on */
    bool     force_stack_spill = false; /* HAR_FORCE_STACK_SPILL (presence) */
    bool     first_vertex = true;       /* HAR_FIRST_VERTEX=0: raygen stores the full path state */
    int      material_queues = -1;      /* HAR_MATERIAL_QUEUES: -1 the integrator's setting, 0 off, else on */
    uint32_t sort_window = 8;           /* HAR_SORT_WINDOW: max(1, .) */
    uint32_t trace_grid = 0;            /* HAR_TRACE_GRID: rounded down to a multiple of the shards, at least the shards; 0 = HAR_MAX_TRAVERSAL_BLOCKS */
    bool     adjoint_inline = true;     /* HAR_ADJOINT_INLINE=0: item + resolve instead of the in-place commit */
    int      late_overlap = -2;         /* HAR_LATE_OVERLAP: -2 absent, -1 off, >= 0 the first bounce */
    int      packet = -1;               /* HAR_PACKET: < 0 the integrator's setting, 0 off, else on */
    uint32_t packet_budget = 160;       /* HAR_PACKET_BUDGET */
    double   refit_max_inflation = 1.5; /* HAR_REFIT_MAX_INFLATION */
    uint32_t refit_max_steps = 0;       /* HAR_REFIT_MAX_STEPS: 0 = no limit */
    bool     host_tlas_update = false;  /* HAR_HOST_TLAS_UPDATE (presence) */
    int      streams = 0;               /* HAR_STREAMS: 1 / 2 force one / two launch sequences */
    uint32_t dual_frac = 50;            /* HAR_DUAL_FRAC: percent, clamped to 10..90 */
    bool     dual_stagger = false;      /* HAR_DUAL_STAGGER: non-zero = on */
    int      prb_tape = 2;              /* HAR_PRB_TAPE: 0 the lane-indexed replay cache, 1 the state tape, >= 2 the record tape */
    bool     verbose = false;           /* HAR_VERBOSE (presence) */
};

/* the variables parse_switches reads, for the documentation test */
constexpr const char *SWITCH_NAMES[] = {
    "HAR_DEBUG_GUARD", "HAR_DEBUG_SYNC", "HAR_TEXEL_QUEUES", "HAR_TQ_LDS", "HAR_TQ_BPQ", "HAR_OVERLAP", "HAR_FORCE_STACK_SPILL", "HAR_FIRST_VERTEX",
    "HAR_MATERIAL_QUEUES", "HAR_SORT_WINDOW", "HAR_TRACE_GRID", "HAR_ADJOINT_INLINE", "HAR_LATE_OVERLAP", "HAR_PACKET", "HAR_PACKET_BUDGET",
    "HAR_REFIT_MAX_INFLATION", "HAR_REFIT_MAX_STEPS", "HAR_HOST_TLAS_UPDATE", "HAR_STREAMS", "HAR_DUAL_FRAC", "HAR_DUAL_STAGGER", "HAR_PRB_TAPE", "HAR_VERBOSE" };

inline Switches parse_switches(const char *(*get)(const char *)) {
    Switches w;
    const char *v;
    if ((v = get("HAR_DEBUG_GUARD"))) w.debug_guard = atoi(v);
    w.debug_sync = get("HAR_DEBUG_SYNC") != nullptr;
    if ((v = get("HAR_TEXEL_QUEUES"))) w.texel_queues = atoi(v) != 0;
    if ((v = get("HAR_TQ_LDS"))) w.tq_lds = (size_t) atol(v);
    if ((v = get("HAR_TQ_BPQ"))) w.tq_bpq = (uint32_t) atoi(v);
    if ((v = get("HAR_OVERLAP"))) w.overlap = atoi(v);
    w.force_stack_spill = get("HAR_FORCE_STACK_SPILL") != nullptr;
    if ((v = get("HAR_FIRST_VERTEX"))) w.first_vertex = atoi(v) != 0;
    if ((v = get("HAR_MATERIAL_QUEUES"))) w.material_queues = atoi(v);
    if ((v = get("HAR_SORT_WINDOW"))) w.sort_window = (uint32_t) std::max(1, atoi(v));
    if ((v = get("HAR_TRACE_GRID"))) w.trace_grid = (uint32_t) std::max(SWITCH_SHARDS, atoi(v) / SWITCH_SHARDS * SWITCH_SHARDS);
    if ((v = get("HAR_ADJOINT_INLINE"))) w.adjoint_inline = atoi(v) != 0;
    if ((v = get("HAR_LATE_OVERLAP"))) w.late_overlap = atoi(v);
    if ((v = get("HAR_PACKET"))) w.packet = atoi(v);
    if ((v = get("HAR_PACKET_BUDGET"))) w.packet_budget = (uint32_t) atoi(v);
    if ((v = get("HAR_REFIT_MAX_INFLATION"))) w.refit_max_inflation = atof(v);
    if ((v = get("HAR_REFIT_MAX_STEPS"))) w.refit_max_steps = (uint32_t) atoi(v);
    w.host_tlas_update = get("HAR_HOST_TLAS_UPDATE") != nullptr;
    if ((v = get("HAR_STREAMS"))) w.streams = atoi(v);
    if ((v = get("HAR_DUAL_FRAC"))) w.dual_frac = (uint32_t) std::min(90, std::max(10, atoi(v)));
    if ((v = get("HAR_DUAL_STAGGER"))) w.dual_stagger = atoi(v) != 0;
    if ((v = get("HAR_PRB_TAPE"))) w.prb_tape = atoi(v);
    w.verbose = get("HAR_VERBOSE") != nullptr;
    return w;
}

inline const Switches &switches() {
    static const Switches w = parse_switches([](const char *name) -> const char * { return getenv(name); });
    return w;
}

}
