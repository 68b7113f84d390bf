/*
 * switches_lib.cpp -- test tool of tests/test_switches_cpu.py (not a product path): parse_switches (har_switches.h) over a table of (name, text)
 * pairs instead of the environment, and plan_chunk (har_plan.h) over flat arrays of integers.  Built by the test into a temporary directory.
 */
#include "../../mitsuba3_amd/csrc/har_plan.h"
#include <cstring>

using namespace har;

namespace {
const char *const *g_names = nullptr, *const *g_values = nullptr; int g_n = 0;
const char *lookup(const char *name) {
    for (int k = 0; k < g_n; ++k) if (!strcmp(g_names[k], name)) return g_values[k];
    return nullptr;
}
Switches parse(const char *const *names, const char *const *values, int n) { g_names = names; g_values = values; g_n = n; return parse_switches(lookup); }
}

extern "C" {

int sw_name_count(void) { return (int) (sizeof(SWITCH_NAMES) / sizeof(SWITCH_NAMES[0])); }
const char *sw_name(int k) { return SWITCH_NAMES[k]; }

/* out[23]: the fields of Switches in the order of their declaration */
void sw_parse(const char *const *names, const char *const *values, int n, double *out) {
    const Switches w = parse(names, values, n);
    const double f[] = { (double) w.debug_guard, (double) w.debug_sync, (double) w.texel_queues, (double) w.tq_lds, (double) w.tq_bpq, (double) w.overlap, (double) w.force_stack_spill,
                         (double) w.first_vertex, (double) w.material_queues, (double) w.sort_window, (double) w.trace_grid, (double) w.adjoint_inline, (double) w.late_overlap,
                         (double) w.packet, (double) w.packet_budget, w.refit_max_inflation, (double) w.refit_max_steps, (double) w.host_tlas_update, (double) w.streams,
                         (double) w.dual_frac, (double) w.dual_stagger, (double) w.prb_tape, (double) w.verbose };
    memcpy(out, f, sizeof(f));
}

/* set[10]: max_depth, rr_depth, hide_emitters, material_queues, packet_tracing, grad_emitters, grad_bsdf_params, grad_light_texels, alpha_film, batch.n (buffers: non-null or null)
 * facts[5]: stack_need, lds_stack, mat_classes, bsdf_types, env_emitter
 * job[14]: mode, cache_mode, n, spp, lane_base, nb, rays, valid_lane, pass_rng, projection, forward_mode, shape_on, adjoint_image, alpha_lane
 * out[15]: mq_on, first_regen, use_mq, overlap, late_on, late_from, inline_commit, spill, shape, fwd, packet, alpha_flags, grid, tgrid, shade_flags */
void sw_plan(const char *const *names, const char *const *values, int n, const long long *set, const long long *facts, const long long *job, long long *out) {
    static float buffer[1];
    const Switches w = parse(names, values, n);
    Settings s;
    s.max_depth = (uint32_t) set[0]; s.rr_depth = (uint32_t) set[1]; s.hide_emitters = set[2] != 0; s.material_queues = set[3] != 0; s.packet_tracing = (int) set[4];
    s.grad_emitters = set[5] ? buffer : nullptr; s.grad_bsdf_params = set[6] ? buffer : nullptr; s.grad_light_texels = set[7] != 0; s.alpha_film = set[8] ? buffer : nullptr;
    s.batch.n = (uint32_t) set[9];
    const SceneFacts f{ (uint32_t) facts[0], (uint32_t) facts[1], (uint32_t) facts[2], (uint32_t) facts[3], (int32_t) facts[4] };
    const ChunkJob j{ (int) job[0], (CacheMode) job[1], (uint32_t) job[2], (uint32_t) job[3], (uint32_t) job[4], (uint32_t) job[5], job[6] != 0, job[7] != 0, job[8] != 0,
                      (uint32_t) job[9], job[10] != 0, job[11] != 0, job[12] != 0, job[13] != 0 };
    const ChunkPlan p = plan_chunk(w, s, f, j);
    const long long r[] = { p.mq_on, p.first_regen, p.use_mq, p.overlap, p.late_on, p.late_from, p.inline_commit, p.spill, p.shape, p.fwd, p.packet, p.alpha_flags, p.grid, p.tgrid, p.shade_flags };
    memcpy(out, r, sizeof(r));
}

}
