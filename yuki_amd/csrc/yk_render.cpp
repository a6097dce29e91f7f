// yk_render.cpp — the batch scheduler that drives the wavefront kernels, behind the C ABI's render entry points.
//
// The scheduler plays the role of the reference's RenderManager/RenderWorker
// pair (renderer/render_manager.rs:69-193, render_worker.rs:62-137): instead of
// num_cpus-1 threads popping 16x16 tiles, ALL pixels x samples of the submitted
// tiles become one work range that is cut into batches of `batch_paths` camera
// samples; each batch runs raygen + max_depth x (trace, shade, shadow,
// accumulate) without any host synchronisation — queue lengths live in device
// memory and the persistent kernels read them there.
//
// Order of the file: the work buffers and run_bounces (one batch's bounce loop; yk_stages.cpp uses them too), the
// interruption helpers, then one submission — a RenderRequest (what an entry point asks for), the plan made of it before
// the device is touched (yk_render_plan.h: pixel offsets, accumulation rules, chunks, batch, work sets) and the phases
// render_tiles_impl runs in order: check_and_plan, the hand-over from a caller's stream, grow_buffers, begin_call, per
// chunk make_pixel_tables and per batch gate_on_cancel + enqueue_batch, the resolve, finish_call — then what yk_li and
// yk_li_debug share (LiCall), and last the entry points in one extern "C" block.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "yk_adaptive.h"
#include "yk_albedo.h"
#include "yk_film_call.h"
#include "yk_guides_through.h"
#include "yk_render_plan.h"
#include "yk_staging.h"
#ifdef YK_EXPERIMENT_SORT  // timing builds only (tools/build_variant.sh sort -DYK_EXPERIMENT_SORT): DESIGN.md §9
#include "../../tools/micro/ray_sort_experiment.h"
#endif
#ifdef YK_EXPERIMENT_GRAPH
#include "../../tools/micro/graph_replay_experiment.h"
#endif

// ------------------------------------------------------------------ render
// ctx->counters: 8 x u64 (closest-hit rays, shadow rays, ...) followed by a 4-word error block whose word
// YK_CTRL_ERR the traversal kernels set on a stack overflow.  Both are zeroed ONCE per call (begin_call) — the
// per-batch control blocks of the work sets are zeroed with every batch and must not hold the flag.
unsigned* error_block(yk_context* ctx) { return reinterpret_cast<unsigned*>(ctx->counters.as<unsigned long long>() + 16); }
CancelRef cancel_ref(yk_context* ctx) { return CancelRef{ctx->cancel_host_dev, ctx->cancel_host_dev ? error_block(ctx) + YK_CTRL_CANCELLED : nullptr}; }

yk_status ensure_work_buffers(yk_context* ctx, WorkSet& ws, size_t paths, unsigned n_lights, unsigned n_delta_lights) {
    HIP_TRY(ctx, ctx->counters.ensure(YK_COUNTER_BYTES));
    unsigned nl = std::max(1u, n_lights);
    unsigned na = nl, nd = std::max(1u, n_delta_lights);  // queue 1 holds every light's rays on the bounces that are not split
    if (paths <= ws.cap_paths && nl <= ws.cap_lights && na <= ws.cap_area && nd <= ws.cap_delta) return YK_OK;
    paths = std::max(paths, ws.cap_paths);
    nl = std::max(nl, ws.cap_lights);
    na = std::max(na, ws.cap_area);
    nd = std::max(nd, ws.cap_delta);
    for (int a = 0; a < 2; ++a)
        for (int b = 0; b < 4; ++b) HIP_TRY(ctx, ws.path[a][b].ensure(paths * 16));
    HIP_TRY(ctx, ws.hit.ensure(paths * 4));
    HIP_TRY(ctx, ws.pend.ensure(paths * 16));
    HIP_TRY(ctx, ws.shC.ensure(paths * nl * 16));
    HIP_TRY(ctx, ws.vis.ensure(paths * YK_VIS_STRIDE(nl)));
    // two shadow queues: rays towards area lights / towards point, spot and distant lights
    HIP_TRY(ctx, ws.shO.ensure(paths * na * 16));
    HIP_TRY(ctx, ws.shD.ensure(paths * na * 16));
    HIP_TRY(ctx, ws.shq.ensure(paths * na * 4));
    HIP_TRY(ctx, ws.shO2.ensure(paths * nd * 16));
    HIP_TRY(ctx, ws.shD2.ensure(paths * nd * 16));
    HIP_TRY(ctx, ws.shq2.ensure(paths * nd * 4));
    HIP_TRY(ctx, ws.ctrl.ensure(YK_CTRL_ALLOC_WORDS * 4));
    ws.cap_paths = paths;
    ws.cap_lights = nl;
    ws.cap_area = na;
    ws.cap_delta = nd;
    return YK_OK;
}

unsigned trace_grid(const yk_context* ctx) { return (unsigned)ctx->n_cu * trace_blocks_per_cu(); }

yk_status ensure_spill(yk_context* ctx, WorkSet& ws) {
    size_t threads = (size_t)trace_grid(ctx) * trace_block_size();
    HIP_TRY(ctx, ws.spill.ensure(threads * trace_spill_depth() * 8));
    HIP_TRY(ctx, ws.spill_side.ensure(threads * trace_spill_depth() * 8));
    return YK_OK;
}

PathBuffers path_buffers(WorkSet& ws, int which) {
    PathBuffers p;
    p.rayO = ws.path[which][0].as<float4>();
    p.rayD = ws.path[which][1].as<float4>();
    p.thru = ws.path[which][2].as<float4>();
    p.rngs = ws.path[which][3].as<uint4>();
    return p;
}

// The queues of bounce b of the batch in `ws` (yk_device.h: BounceQueues, and the control block's words: the only place
// that knows which word belongs to which queue).
static BounceQueues bounce_queues(WorkSet& ws, unsigned b) {
    unsigned* bc = ws.ctrl.as<unsigned>() + YK_CTRL_BOUNCE(b);  // this bounce's counters and queue heads, zeroed with the batch
    BounceQueues q;
    q.hit = ws.hit.as<int>();
    q.pend = ws.pend.as<float4>();
    q.shC = ws.shC.as<float4>();
    q.vis = ws.vis.as<unsigned char>();
    q.area = ShadowQueue{ws.shO.as<float4>(), ws.shD.as<float4>(), ws.shq.as<unsigned>(), bc + YK_CTRL_SHQ, bc + YK_CTRL_HEAD + 1};
    q.delta = ShadowQueue{ws.shO2.as<float4>(), ws.shD2.as<float4>(), ws.shq2.as<unsigned>(), bc + YK_CTRL_SHQ2, bc + YK_CTRL_HEAD + 2};
    q.count = bc;
    q.next_count = bc + YK_CTRL_STRIDE;
    q.closest_head = bc + YK_CTRL_HEAD;
    return q;
}

yk_status make_params(yk_context* ctx, const yk_sampler_desc* smp, const yk_integrator_desc* integ, RenderParams& prm) {
    if (!smp || !integ) return fail(ctx, YK_ERR_INVALID_ARGUMENT, "null sampler/integrator");
    std::memset(&prm, 0, sizeof(prm));
    prm.sampler.kind = smp->kind;
    prm.sampler.nx = smp->nx;
    prm.sampler.ny = smp->kind == YK_SAMPLER_UNIFORM ? 1 : smp->ny;
    prm.sampler.jitter = smp->jitter;
    prm.sampler.seed = smp->seed;
    if (smp->kind > 1 || prm.sampler.nx == 0 || prm.sampler.ny == 0) return fail(ctx, YK_ERR_INVALID_ARGUMENT, "bad sampler");
    uint64_t spp = (uint64_t)prm.sampler.nx * prm.sampler.ny;
    if (spp > 0xFFFFu) return fail(ctx, YK_ERR_INVALID_ARGUMENT, "samples per pixel exceed u16 (integrators/mod.rs:139)");
    prm.sampler.spp = (unsigned)spp;
    prm.spe = (unsigned)spp;  // plain film: every sample of the pixel (callers with a sample-index table overwrite it)
    prm.max_depth = integ->max_depth;
    prm.has_clamp = integ->has_clamp;
    prm.clamp = integ->indirect_clamp;
    prm.integrator = integ->kind;
    prm.nee_skip = ctx ? (uint32_t)ctx->nee_skip : 0u;
    if (integ->kind == YK_INTEGRATOR_WHITTED && integ->max_depth > whitted_max_depth())
        return fail(ctx, YK_ERR_UNSUPPORTED, "Whitted: max_depth above 16 is not supported on the device");
    if (integ->kind > YK_INTEGRATOR_SHADING_UVS) return fail(ctx, YK_ERR_INVALID_ARGUMENT, "bad integrator kind");
    return YK_OK;
}


// camera rays (and the leading bounces the "packet_bounces" option names) go to the wave-packet kernel
bool packet_kernel_traces_bounce(const yk_context* ctx, const yk_scene* scene, unsigned b) {
    return b < (unsigned)ctx->packet_bounces && scene->bvh->depth <= 64;
}

// one batch of `n` paths already generated into buffer 0; runs the bounce loop
void run_bounces(yk_context* ctx, WorkSet& ws, hipStream_t st, const yk_scene* scene, const RenderParams& prm, const uint32_t* pixel_xy,
                        const uint32_t* sample_index_tab, float4* sample_buf, KernelTimer& kt, unsigned long long* counters, bool coherent,
                        uint32_t n_paths, uint32_t sid_base, bool lean_camera_bounce, uint32_t* n_shadow_launches) {
    unsigned* ctrl = ws.ctrl.as<unsigned>();
    unsigned* errblk = error_block(ctx);  // outlives the batch (ctrl is zeroed per batch)
    // Two node layouts: the binary 64-byte nodes win when the machine is full (one 4-wide node
    // costs the loads of two binary ones, and throughput is bound by per-lane loads);
    // the 4-wide collapse halves the dependent steps of a ray, which is what a job too small to
    // fill the machine waits for (a 16x16 tile: 1.83 -> 1.38 ms, a 1080p pass: 7.7 -> 7.0 ms,
    // equal at 8 M paths, 9 % slower for the 132 M-path frame).
    const DevScene ds = dev_scene_for(scene, n_paths);
    // Queue lengths are only known on the device, but none exceeds the batch's path count
    // (x lights for shadow rays).  A small job — one 16x16 tile of the reference's per-tile
    // calls is 16 K paths — gets grids of that size instead of machine-filling ones: every wave
    // of a persistent kernel pays one atomic on the queue head before it can find out that
    // there is nothing for it (7168 waves x 8 bounces x 3 kernels per tile otherwise).
    auto fit = [](unsigned full, uint64_t items) { return (unsigned)std::min<uint64_t>(full, std::max<uint64_t>(1, (items + 255) / 256)); };
    const uint64_t n_shadow_max = (uint64_t)n_paths * std::max(1u, scene->n_lights);
    const unsigned tg = fit(trace_grid(ctx), n_paths), tg_any = fit(trace_grid(ctx), n_shadow_max);
    const unsigned pg_full = (unsigned)ctx->n_cu * packet_blocks_per_cu();
    const unsigned pg = fit(pg_full, n_paths), pg_any = fit(pg_full, n_shadow_max);
    // k_shade / k_accumulate are grid-stride kernels: 256 blocks per CU (three are resident) let the block
    // scheduler even out the iterations' very different costs; 8 persistent-style blocks per CU were 2.9 % slower
    // on the frame (sweep 3..1024: 147.3, 146.9, 148.0 (8), 146.6, 145.4 (24), 145.1 (96), 143.7 (256), 144.2, 144.3 ms)
    static const unsigned shade_bpc = std::getenv("YK_SHADE_BPC") ? (unsigned)std::atoi(std::getenv("YK_SHADE_BPC")) : 256u;
    const unsigned sg = fit((unsigned)ctx->n_cu * shade_bpc, n_paths);  // k_accumulate: 256 paths per block and step
    const unsigned spill_stride = trace_grid(ctx) * trace_block_size();
    unsigned cur = 0;
    unsigned long long debug_reported = 0;  // YK_DEBUG_BOUNCES: the render's shadow-ray count when the bounce began
    if (kt.on && std::getenv("YK_DEBUG_BOUNCES")) {
        (void)hipDeviceSynchronize();
        (void)hipMemcpy(&debug_reported, counters + 1, sizeof(debug_reported), hipMemcpyDeviceToHost);
    }
    // Bounce b: trace_closest -> shade on `st`; then {trace_any, accumulate}(b) go to the side
    // stream while `st` already traces bounce b+1 — two persistent kernels whose drained
    // CUs are picked up by the other one (the tail of a small launch is one long ray).
    // shade(b+1) overwrites what accumulate(b) reads (the other path buffer, pend, shC, vis,
    // the shadow queue and its counter), so it waits for ev_acc.
    const bool overlap = ctx->overlap_shadow != 0 && ws.side != nullptr;
    hipStream_t sb = overlap ? ws.side : st;
    for (unsigned b = 0; b < prm.max_depth; ++b) {
        PathBuffers pc = path_buffers(ws, (int)cur), pn = path_buffers(ws, (int)(cur ^ 1u));
        // camera rays (consecutive samples of a pixel) and the shadow rays they spawn are coherent:
        // the wave walks the tree once for all 64 of them (yk_packet.hip)
        const bool packet = coherent && packet_kernel_traces_bounce(ctx, scene, b);
        // lean camera bounce (yk_device.h, YK_CTRL_CAM_O): raygen stored neither origins nor throughputs
        const float4* lean_origin = (b == 0 && lean_camera_bounce) ? reinterpret_cast<const float4*>(ctrl + YK_CTRL_CAM_O) : nullptr;
        const bool packet_shadow = coherent && b < (unsigned)ctx->packet_shadow_bounces && scene->bvh->depth <= 64 && scene->n_delta_lights > 0;
        // shadow rays are split into two queues only when the second one gets the packet kernel;
        // otherwise everything goes to the first queue and one launch traces it
        const bool split = packet_shadow && scene->n_lights > scene->n_delta_lights;
        const bool all_delta = packet_shadow && !split;  // no area lights: the single queue is all coherent
        BounceQueues q = bounce_queues(ws, b);
        int e = kt.begin(st);
        if (packet)
            launch_trace_closest_packet(st, pg, ds, lean_origin ? nullptr : pc.rayO, pc.rayD, q.count, q.closest_head, q.hit, counters, lean_origin, prm.cancel);
        else {
            launch_trace_closest(st, tg, ds, pc.rayO, pc.rayD, nullptr, q.count, q.closest_head, q.hit, nullptr, nullptr,
                                 ws.spill.as<uint2>(), spill_stride, errblk, counters, prm.cancel.host);
        }
        kt.end(e, 0, st);
        if (overlap && b > 0) (void)hipStreamWaitEvent(st, ws.ev_acc, 0);
        e = kt.begin(st);
        launch_shade(st, sg, ds, prm, pixel_xy, sample_index_tab, pc, pn, q, split ? 1u : 0u, (b > 0 && ctx->shade_reorder) ? 1u : 0u, 3u * (unsigned)ctx->n_cu,
                     sid_base, lean_origin, counters + 1);
        kt.end(e, 2, st);
#ifdef YK_EXPERIMENT_SORT  // order the queues k_shade just wrote (synchronises: timing experiment, tools/micro/ray_sort_experiment.h)
        YK_SORT_AFTER_SHADE
#endif
        if (overlap) {
            (void)hipEventRecord(ws.ev_shade, st);
            (void)hipStreamWaitEvent(sb, ws.ev_shade, 0);
        }
        e = kt.begin(sb);
        uint2* any_spill = (overlap ? ws.spill_side : ws.spill).as<uint2>();
        if (all_delta) {
            launch_trace_any_packet(sb, pg_any, ds, q.area, q.vis, counters + 1, prm.cancel);
        } else {
            launch_trace_any(sb, tg_any, ds, q.area, q.vis, any_spill, spill_stride, errblk, counters + 1, prm.cancel.host);
            if (split && n_shadow_launches) ++*n_shadow_launches;
            if (split)  // rays converging on a point / spot / distant light: wave packets
                launch_trace_any_packet(sb, pg_any, ds, q.delta, q.vis, counters + 1, prm.cancel);
        }
        kt.end(e, 1, sb);
        if (n_shadow_launches) ++*n_shadow_launches;
        launch_accumulate(sb, sg, prm, pc, q, ds.n_lights, sample_buf, b == 0 ? 1u : 0u, sid_base);
        if (overlap) (void)hipEventRecord(ws.ev_acc, sb);
        if (kt.on && std::getenv("YK_DEBUG_BOUNCES")) {  // per-bounce breakdown (synchronises; diagnostics only)
            unsigned h[YK_CTRL_STRIDE + 1];
            (void)hipDeviceSynchronize();  // the other work set's batch as well: the shadow counter is the context's
            (void)hipMemcpy(h, q.count, sizeof(h), hipMemcpyDeviceToHost);  // the bounce's words of the control block (yk_device.h)
            // traced: what the any-hit queues held; reported: what the bounce added to the render's shadow-ray count, the queues and
            // the rays k_shade left out because they add +-0 ("nee_skip" bit 2)
            unsigned long long reported_now = 0;
            (void)hipMemcpy(&reported_now, counters + 1, sizeof(reported_now), hipMemcpyDeviceToHost);
            std::fprintf(stderr, "bounce %u: shadow rays traced / reported %u / %llu\n", b, h[YK_CTRL_SHQ] + h[YK_CTRL_SHQ2], reported_now - debug_reported);
            debug_reported = reported_now;
            float tt = 0, ts = 0, th = 0;
            (void)hipEventElapsedTime(&tt, ctx->ev_pool[kt.spans[0].back().first], ctx->ev_pool[kt.spans[0].back().second]);
            (void)hipEventElapsedTime(&ts, ctx->ev_pool[kt.spans[1].back().first], ctx->ev_pool[kt.spans[1].back().second]);
            (void)hipEventElapsedTime(&th, ctx->ev_pool[kt.spans[2].back().first], ctx->ev_pool[kt.spans[2].back().second]);
            std::fprintf(stderr, "bounce %u: rays %u trace %.3f ms (%.0f Mray/s) | shadow rays %u %.3f ms (%.0f Mray/s) | shade %.3f ms | survivors %u\n", b, h[0],
                         tt, h[0] / (tt * 1e3), h[YK_CTRL_SHQ] + h[YK_CTRL_SHQ2], ts, (h[YK_CTRL_SHQ] + h[YK_CTRL_SHQ2]) / (ts * 1e3), th, h[YK_CTRL_STRIDE]);
        }
        cur ^= 1u;
    }
    if (overlap) (void)hipStreamWaitEvent(st, ws.ev_acc, 0);  // the batch is complete on `st` once its last accumulate is
}

// ------------------------------------------------------------------ interruption (yk_device.h, CancelRef)
// Raise the host's word: every traversal launch's relay wave sees it at its next claim (yk_device.h, CancelRef) and raises the
// device word that every later launch reads when it starts.
static double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
static const bool g_debug_cancel = std::getenv("YK_DEBUG_CANCEL") != nullptr;

static void raise_cancel(yk_context* ctx, bool from_render_thread = true) {
    if (!ctx->cancel_host) return;
    const double t0 = g_debug_cancel ? now_ms() : 0.0;
    ctx->cancel_raised.store(true, std::memory_order_release);
    __atomic_store_n(ctx->cancel_host, 1u, __ATOMIC_RELEASE);
    // ... and the device word directly (a copy engine's job: it does not queue behind the kernels): k_shade looks at this one only.
    // The stream that carries the copy is NOT made here — the first interruption of a context relies on the relay wave alone (the
    // device word is up one traversal launch later at most) and leaves a note; the stream is created when the next submission
    // clears the word (clear_cancel), off the path whose latency the caller is waiting on.
    if (from_render_thread && !ctx->cancel_stream) ctx->want_cancel_stream = true;
    if (from_render_thread && ctx->cancel_stream && ctx->counters.p)
        (void)hipMemcpyAsync(error_block(ctx) + YK_CTRL_CANCELLED, ctx->cancel_host + 16, 4, hipMemcpyHostToDevice, ctx->cancel_stream);
    if (g_debug_cancel) std::fprintf(stderr, "[yk cancel] raise: %s, %.3f ms\n", ctx->cancel_stream ? "host word + device word" : "host word only (first interruption)", now_ms() - t0);
}

// Called by a submission before it enqueues anything: if an earlier one was interrupted, whatever it still has on the
// context's streams drains first — the word may only be cleared when no kernel that honoured it can run again.
static yk_status clear_cancel(yk_context* ctx) {
    if (!ctx->cancel_host || !ctx->cancel_raised.load(std::memory_order_acquire)) return YK_OK;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (ctx->cancel_stream) HIP_TRY(ctx, hipStreamSynchronize(ctx->cancel_stream));  // a late copy of the 1 must not land in the next submission
    for (WorkSet& w : ctx->ws) {
        if (w.stream && w.stream != ctx->stream) HIP_TRY(ctx, hipStreamSynchronize(w.stream));
        if (w.side) HIP_TRY(ctx, hipStreamSynchronize(w.side));
    }
    __atomic_store_n(ctx->cancel_host, 0u, __ATOMIC_RELEASE);
    ctx->cancel_raised.store(false, std::memory_order_release);
    if (ctx->want_cancel_stream && !ctx->cancel_stream) {  // this context gets interrupted: later interruptions also write the device word directly
        if (hipStreamCreateWithFlags(&ctx->cancel_stream, hipStreamNonBlocking) != hipSuccess) ctx->cancel_stream = nullptr;
        ctx->want_cancel_stream = false;
    }
    return YK_OK;
}

// Wait for `done` (recorded on the stream that ends the submission) while polling the caller's predicate about every
// 100 us — the reference polls it once per pixel sample (integrators/mod.rs:153; render_worker.rs:240-255 relies on
// that for "low latency kills").  Returns true when the predicate fired: the word is raised and the streams have drained.
static bool poll_until(yk_context* ctx, hipEvent_t done, yk_cancel_fn cancel, void* user) {
    while (hipEventQuery(done) == hipErrorNotReady) {
        if (cancel(user)) {
            raise_cancel(ctx);
            return true;
        }
        std::this_thread::sleep_for(std::chrono::microseconds(100));
    }
    return false;
}
static bool wait_polling(yk_context* ctx, hipEvent_t done, hipStream_t st, yk_cancel_fn cancel, void* user) {
    const bool fired = cancel ? poll_until(ctx, done, cancel, user) : false;
    (void)hipStreamSynchronize(st);
    return fired;
}

// ------------------------------------------------------------------ what the entry points share
// The four words of the error block, read back, as the call's verdict.
static yk_status error_block_status(yk_context* ctx, const unsigned* words) {
    if (words[YK_CTRL_ERR] & 1u) return fail(ctx, YK_ERR_STACK_OVERFLOW, "BVH traversal stack exceeded 64 entries (bvh.rs:174)");
    return YK_OK;
}

// tiles -> pixel offsets (yk_render_plan.h); `too_many`: how this caller says that they exceed 32 bits
static yk_status tile_offsets(yk_context* ctx, const yk_tile* tiles, size_t n_tiles, std::vector<uint32_t>& off, const char* too_many) {
    switch (yk_plan::tile_ranges(tiles, n_tiles, off)) {
        case yk_plan::TILES_OK: return YK_OK;
        case yk_plan::TILES_TOO_MANY_PIXELS: return fail(ctx, YK_ERR_INVALID_ARGUMENT, too_many);
        default: return fail(ctx, YK_ERR_INVALID_ARGUMENT, "Bounds2 with a dimension <= 0");
    }
}

// ------------------------------------------------------------------ one render submission
// Integrator::render for a list of tiles, as every render entry point asks for it: each fills in what it means.
struct RenderRequest {
    const yk_scene* scene = nullptr;
    const yk_camera* camera = nullptr;
    const yk_sampler_desc* sampler = nullptr;
    const yk_integrator_desc* integrator = nullptr;
    const yk_tile* tiles = nullptr;
    size_t n_tiles = 0;
    // NULL: the plain film (all samples of a pixel, mean stored).  Otherwise the accumulating film (integrators/mod.rs:
    // 146-161): passes FilmTile.sample .. + n_passes - 1 of every tile, raw values stored pass-major.
    const uint16_t* tile_samples = nullptr;
    const yk_tile_list* list = nullptr;  // instead of the three above: a prepared list, its pixel table on the device already
    // instead of tiles altogether: a pixel list (yk_adaptive.h) — every entry its own first sample index, n_passes of them
    // rendered, the accumulating film.  With d_film_sum and d_stats (a film_res_x-wide film of sums and its yk_pixel_stats)
    // instead of d_out, every chunk's samples are folded straight into them (k_ad_fold) and no pass-major buffer exists.
    const yk_pixel_list* pixels = nullptr;
    void* d_film_sum = nullptr;
    void* d_stats = nullptr;
    uint32_t n_passes = 1;
    int64_t uniform_first_sample = -1;  // >= 0: the accumulating film with this first sample index for every tile
    void* d_out = nullptr;
    // != 0: the guide pass (yk_render_guides) — a debug integrator's trace, one sample a pixel; d_out is then a row-major
    // film of yk_guide records, guides_res_x wide, written by k_guides instead of the shade and resolve kernels.  With
    // d_ids (yk_render_guides_ids) k_guides_ids writes the yk_surface_id records there too, and d_out may be NULL.
    // With ids_band_rows != 0 (yk_render_albedo_mean) the tiles are rows [ids_row0, ids_row0 + ids_band_rows) of the film and
    // d_ids is a buffer of that band alone: k_ids_band writes the ids at their place in the band, and no guides.
    uint32_t guides_res_x = 0;
    void* d_ids = nullptr;
    uint32_t ids_row0 = 0, ids_band_rows = 0;
    // through (yk_render_guides_through, yk_guides_through.h): the guide pass follows glass for up to max_through
    // interfaces — k_guides_step instead of k_guides after every trace; d_out, d_ids and d_through (one uint32 a pixel: the
    // interfaces crossed) may each be NULL, not all three.
    bool through = false;
    uint32_t max_through = 0;
    void* d_through = nullptr;
    void* stream = nullptr;
    yk_render_stats* stats = nullptr;
    yk_cancel_fn cancel = nullptr;
    void* user = nullptr;
};
// what the tile entry points of the ABI pass through as they got it, in the ABI's order; the tiles are theirs to fill in
static RenderRequest request_for(const yk_scene* scene, const yk_camera* camera, const yk_sampler_desc* sampler, const yk_integrator_desc* integrator,
                                 void* d_out_rgb, void* stream, yk_render_stats* stats, yk_cancel_fn cancel, void* user) {
    RenderRequest rq;
    rq.scene = scene;
    rq.camera = camera;
    rq.sampler = sampler;
    rq.integrator = integrator;
    rq.d_out = d_out_rgb;
    rq.stream = stream;
    rq.stats = stats;
    rq.cancel = cancel;
    rq.user = user;
    return rq;
}

// The phases of a submission in the order render_tiles_impl runs them, over what they share.
struct Submission {
    yk_context* const ctx;
    const RenderRequest& rq;
    const yk_scene* const scene;
    const yk_tile* tiles;  // the request's, or its prepared list's
    const uint16_t* tile_samples;
    size_t n_tiles;
    std::vector<uint32_t> own_off;
    const uint32_t* off = nullptr;  // n_tiles + 1 pixel offsets: the prepared list's, or own_off
    const hipStream_t st;           // the render always runs on the context's own streams (render_tiles_impl: the hand-over)
    yk_plan::RenderPlan plan;
    RenderParams prm;
    DevCamera cam;
    bool is_path = false;
    KernelTimer kt;
    struct EventPair {  // destroyed on every exit path
        hipEvent_t a = nullptr, b = nullptr;
        ~EventPair() {
            if (a) (void)hipEventDestroy(a);
            if (b) (void)hipEventDestroy(b);
        }
    } frame_ev;
    uint32_t n_batches = 0, n_trace = 0, n_shadow = 0;
    // the chunk in progress
    float4* sample_buf = nullptr;
    uint32_t* pixel_xy = nullptr;
    uint32_t* pixel_sample = nullptr;
    int which = 0;
    bool ws_busy[2] = {false, false};

    Submission(yk_context* c, const RenderRequest& r) : ctx(c), rq(r), scene(r.scene), tiles(r.tiles), tile_samples(r.tile_samples), n_tiles(r.n_tiles), st(c->stream) {}
    unsigned long long* counters() const { return ctx->counters.as<unsigned long long>(); }

    // the arguments, then — nothing of it touches the device — the plan
    yk_status check_and_plan() {
        if (rq.list) {
            if (rq.list->device != ctx->device) return fail(ctx, YK_ERR_INVALID_ARGUMENT, "tile list was not created on this context's device");
            tiles = rq.list->tiles.data();
            tile_samples = rq.list->samples.empty() ? nullptr : rq.list->samples.data();
            n_tiles = rq.list->tiles.size();
        }
        if (rq.pixels) {
            if (rq.pixels->ctx != ctx) return fail(ctx, YK_ERR_INVALID_ARGUMENT, "pixel list was not created on this context");
            if (!scene || !rq.camera || (!rq.d_out && !(rq.d_film_sum && rq.d_stats))) return fail(ctx, YK_ERR_INVALID_ARGUMENT, "null argument");
        } else if (!scene || !rq.camera || !tiles || n_tiles == 0 || (!rq.d_out && !(rq.guides_res_x && (rq.d_ids || rq.d_through))))
            return fail(ctx, YK_ERR_INVALID_ARGUMENT, "null argument");
        if (yk_status rs = scene_on_context(ctx, scene, "")) return rs;
        yk_status rc = make_params(ctx, rq.sampler, rq.integrator, prm);
        if (rc != YK_OK) return rc;
        is_path = prm.integrator == YK_INTEGRATOR_PATH;
        if (is_path && prm.max_depth > YK_CTRL_MAX_DEPTH) return fail(ctx, YK_ERR_INVALID_ARGUMENT, "max_depth too large");
        (void)hipSetDevice(ctx->device);
        if ((rc = clear_cancel(ctx)) != YK_OK) return rc;
        const char* refusal = nullptr;
        if (rq.pixels) {
            refusal = plan.set_pixel_list(rq.pixels->n, rq.n_passes, rq.pixels->passes, rq.pixels->sample_end, prm.sampler.spp, (uint64_t)ctx->sample_buf_cap);
        } else {
            if (!rq.list && (rc = tile_offsets(ctx, tiles, n_tiles, own_off, "too many pixels in one call")) != YK_OK) return rc;
            off = rq.list ? rq.list->off.data() : own_off.data();  // a list's were validated when it was made
            refusal = plan.set_samples(tile_samples, n_tiles, rq.uniform_first_sample, rq.n_passes, prm.sampler.spp);
            if (!refusal) refusal = plan.set_chunks(off, n_tiles, (uint64_t)ctx->sample_buf_cap);
        }
        if (refusal) return fail(ctx, YK_ERR_INVALID_ARGUMENT, refusal);
        plan.set_batch((uint64_t)ctx->batch_paths, ctx->streams, is_path, rq.stream != nullptr);
        prm.spe = plan.spp;
        prm.sample_base = plan.sample_base;
        std::memcpy(cam.c2w, rq.camera->camera_to_world, 64);
        std::memcpy(cam.r2c, rq.camera->raster_to_camera, 64);
        return YK_OK;
    }

    yk_status grow_buffers() {
        size_t free_b = 0, total_b = 0;
        if (plan.batch > ctx->ws[0].cap_paths && hipMemGetInfo(&free_b, &total_b) == hipSuccess) plan.clamp_batch_to_hbm(free_b, scene->n_lights);
        if (plan.n_ws == 2 && !ctx->ws[1].stream) {  // the second work set's stream pair, on first use
            HIP_TRY(ctx, hipStreamCreateWithFlags(&ctx->ws[1].stream, hipStreamNonBlocking));
            HIP_TRY(ctx, hipStreamCreateWithFlags(&ctx->ws[1].side, hipStreamNonBlocking));
        }
        for (int w = 0; w < plan.n_ws; ++w) {
            yk_status wb = ensure_work_buffers(ctx, ctx->ws[w], plan.batch, scene->n_lights, scene->n_delta_lights);
            if (wb != YK_OK) return wb;
            if ((wb = ensure_spill(ctx, ctx->ws[w])) != YK_OK) return wb;
        }
        HIP_TRY(ctx, ctx->tiles.ensure(n_tiles * sizeof(yk_tile)));
        HIP_TRY(ctx, ctx->tile_off.ensure((n_tiles + 1) * 4));
        if (prm.integrator == YK_INTEGRATOR_BVH_INTERSECTIONS) HIP_TRY(ctx, ctx->stats4.ensure(plan.batch * 16));
        return YK_OK;
    }

    yk_status begin_call() {
        HIP_TRY(ctx, hipMemsetAsync(counters(), 0, YK_COUNTER_BYTES, st));  // the error block with it: stack-overflow flag, interruption word
        prm.cancel = cancel_ref(ctx);
        kt.ctx = ctx;
        // per-kernel HIP-event timings: two event records per launch and one elapsed-time query per
        // kernel — not for jobs so small (a tile, a few tiles) that this bookkeeping is the cost
        kt.on = rq.stats != nullptr && ctx->time_kernels != 0 && (plan.total_work >= (1u << 20) || ctx->time_kernels > 1);
        if (rq.stats) {
            HIP_TRY(ctx, hipEventCreate(&frame_ev.a));
            HIP_TRY(ctx, hipEventCreate(&frame_ev.b));
            HIP_TRY(ctx, hipEventRecord(frame_ev.a, st));
        }
        return YK_OK;
    }

    // the chunk's pixel table (and, with a sample table, its per-pixel sample indices) on the device, by one of three routes
    yk_status make_pixel_tables(const yk_plan::Chunk& c) {
        const bool sample_table = plan.sample_table;
        const size_t nt = c.t_end - c.t_begin;
        pixel_sample = nullptr;
        if (rq.pixels) {  // the list's two tables are the chunk's, as they are
            pixel_xy = rq.pixels->pixel_xy.as<uint32_t>() + c.px0;
            pixel_sample = rq.pixels->pixel_sample.as<uint32_t>() + c.px0;
            return YK_OK;
        }
        if (rq.list) {  // the pixel table of the whole list is already on the device
            pixel_xy = rq.list->pixel_xy.as<uint32_t>() + c.px0;
            if (sample_table) pixel_sample = rq.list->pixel_sample.as<uint32_t>() + c.px0;
            return YK_OK;
        }
        HIP_TRY(ctx, ctx->pixel_xy.ensure((size_t)c.npx * 4));
        pixel_xy = ctx->pixel_xy.as<uint32_t>();
        if (sample_table) {
            HIP_TRY(ctx, ctx->pixel_sample.ensure((size_t)c.npx * 4));
            pixel_sample = ctx->pixel_sample.as<uint32_t>();
        }
        if (nt == 1) {  // one tile (the reference's per-tile call): it travels as a kernel argument
            launch_pixel_table_one(st, tiles[c.t_begin], c.npx, pixel_xy, sample_table ? tile_samples[c.t_begin] : 0u, pixel_sample);
            return YK_OK;
        }
        std::vector<uint32_t> loc(nt + 1);
        for (size_t t = c.t_begin; t <= c.t_end; ++t) loc[t - c.t_begin] = off[t] - c.px0;
        HIP_TRY(ctx, hipMemcpyAsync(ctx->tiles.p, tiles + c.t_begin, nt * sizeof(yk_tile), hipMemcpyHostToDevice, st));
        HIP_TRY(ctx, hipMemcpyAsync(ctx->tile_off.p, loc.data(), loc.size() * 4, hipMemcpyHostToDevice, st));
        HIP_TRY(ctx, hipStreamSynchronize(st));  // `loc` is a stack-lifetime staging buffer
        const uint16_t* d_tile_sample = nullptr;
        if (sample_table) {
            HIP_TRY(ctx, ctx->tile_sample.ensure(nt * 2));
            HIP_TRY(ctx, hipMemcpyAsync(ctx->tile_sample.p, tile_samples + c.t_begin, nt * 2, hipMemcpyHostToDevice, st));
            d_tile_sample = ctx->tile_sample.as<uint16_t>();
        }
        launch_pixel_table(st, ctx->tiles.as<yk_tile>(), ctx->tile_off.as<uint32_t>(), (uint32_t)nt, c.npx, pixel_xy, d_tile_sample, pixel_sample);
        return YK_OK;
    }

    // An interruptible job of many batches is not enqueued all at once: a work set takes its next batch when its
    // previous one has finished (the other work set's batch keeps the GPU busy meanwhile), the predicate is polled
    // during the wait, and an interruption has at most two batches' launches left to drain — each of them an empty
    // launch of a few microseconds, but a 4K x 256 spp job holds 1300 of them.
    yk_status gate_on_cancel(WorkSet& ws, uint64_t w0, uint64_t work) {
        if (!rq.cancel) return YK_OK;
        bool fired = ws_busy[which] && poll_until(ctx, ws.ev_batch, rq.cancel, rq.user);
        if (!fired && rq.cancel(rq.user)) {
            raise_cancel(ctx);
            fired = true;
        }
        if (!fired) return YK_OK;
        // what is already enqueued drains at once
        const double t0 = g_debug_cancel ? now_ms() : 0.0;
        (void)hipStreamSynchronize(st);
        const double t1 = g_debug_cancel ? now_ms() : 0.0;
        if (plan.n_ws == 2) (void)hipStreamSynchronize(ctx->ws[1].stream);
        if (g_debug_cancel) {
            unsigned words[4] = {0, 0, 0, 0};
            (void)hipMemcpy(words, error_block(ctx), sizeof words, hipMemcpyDeviceToHost);
            std::fprintf(stderr, "[yk cancel] drain: stream0 %.3f ms, stream1 %.3f ms, batch %llu of %llu, device word %u\n", t1 - t0, now_ms() - t1,
                         (unsigned long long)(w0 / plan.batch), (unsigned long long)((work + plan.batch - 1) / plan.batch), words[YK_CTRL_CANCELLED]);
        }
        return fail(ctx, YK_ERR_CANCELLED, "cancelled by early_termination_predicate");
    }

    // raygen for samples [w0, w0 + n) of the chunk, then the integrator family's kernels, on `bs`
    yk_status enqueue_batch(WorkSet& ws, hipStream_t bs, uint64_t w0, uint32_t n) {
        unsigned* ctrl = ws.ctrl.as<unsigned>();
        unsigned* bc0 = ctrl + YK_CTRL_BOUNCE(0);
        unsigned* errblk = error_block(ctx);
        const unsigned spill_stride = trace_grid(ctx) * trace_block_size();
        PathBuffers pc = path_buffers(ws, 0);
        HIP_TRY(ctx, hipMemsetAsync(ctrl, 0, YK_CTRL_WORDS * 4, bs));
        // Path, camera rays traced by the packet kernel: the lean camera bounce (yk_device.h, YK_CTRL_CAM_O)
        const bool lean = is_path && prm.max_depth > 0 && packet_kernel_traces_bounce(ctx, scene, 0);
        launch_raygen(bs, cam, prm, pixel_xy, pixel_sample, w0, n, pc, sample_buf, bc0, lean ? reinterpret_cast<float4*>(ctrl + YK_CTRL_CAM_O) : nullptr,
                      ctx->pixel_aux.as<uint4>());
        ++n_batches;
        if (is_path) {
            run_bounces(ctx, ws, bs, scene, prm, pixel_xy, pixel_sample, sample_buf, kt, counters(), true, n, (uint32_t)w0, lean, &n_shadow);
            n_trace += prm.max_depth;
            return YK_OK;
        }
        ++n_trace;
        int e = kt.begin(bs);
        if (prm.integrator == YK_INTEGRATOR_WHITTED) {  // one lane per camera sample runs the whole recursion (whitted.rs:74-181)
            launch_whitted(bs, trace_grid(ctx), scene->dev, prm, pixel_xy, pixel_sample, pc, n, sample_buf, ws.spill.as<uint2>(), spill_stride, errblk, counters());
            kt.end(e, 0, bs);
            return YK_OK;
        }
        const bool want_stats = prm.integrator == YK_INTEGRATOR_BVH_INTERSECTIONS;
        launch_trace_closest(bs, trace_grid(ctx), dev_scene_for(scene, n), pc.rayO, pc.rayD, nullptr, bc0, bc0 + YK_CTRL_HEAD, ws.hit.as<int>(), nullptr,
                             want_stats ? ctx->stats4.as<uint4>() : nullptr, ws.spill.as<uint2>(), spill_stride, errblk, counters());
        kt.end(e, 0, bs);
        if (rq.guides_res_x && rq.through) return enqueue_guides_through(ws, bs, n);
        if (rq.guides_res_x && rq.d_ids && rq.ids_band_rows)
            launch_ids_band(bs, scene->dev, pc, ws.hit.as<int>(), n, pixel_xy, rq.guides_res_x, rq.ids_row0, rq.ids_band_rows, reinterpret_cast<uint4*>(rq.d_ids));
        else if (rq.guides_res_x && rq.d_ids)
            launch_guides_ids(bs, scene->dev, pc, ws.hit.as<int>(), n, pixel_xy, rq.guides_res_x, reinterpret_cast<float4*>(rq.d_out), reinterpret_cast<uint4*>(rq.d_ids));
        else if (rq.guides_res_x)
            launch_guides(bs, scene->dev, pc, ws.hit.as<int>(), n, pixel_xy, rq.guides_res_x, reinterpret_cast<float4*>(rq.d_out));
        else
            launch_debug_shade(bs, scene->dev, prm.integrator, pc, ws.hit.as<int>(), ctx->stats4.as<uint4>(), n, sample_buf);
        return YK_OK;
    }

    // The guide pass through glass (yk_guides_through.h) after the batch's camera rays were traced: k_guides_step of pass 0,
    // then per further pass the closest-hit trace of the continuation queue and its k_guides_step.  Pass k's rays live in
    // path buffer k & 1, their count in word 0 of bounce k's control words (raygen wrote bounce 0's, the step before wrote
    // the others into the batch's zeroed block) and the trace's work-queue head beside it; nothing is read back — the later
    // launches are sized for the batch (`n`) and find their count on the device.
    yk_status enqueue_guides_through(WorkSet& ws, hipStream_t bs, uint32_t n) {
        unsigned* ctrl = ws.ctrl.as<unsigned>();
        const DevScene ds = dev_scene_for(scene, n);
        const unsigned tg = (unsigned)std::min<uint64_t>(trace_grid(ctx), std::max<uint64_t>(1, ((uint64_t)n + 255) / 256));
        const unsigned spill_stride = trace_grid(ctx) * trace_block_size();
        for (uint32_t k = 0; k <= rq.max_through; ++k) {
            unsigned* bc = ctrl + YK_CTRL_BOUNCE(k);
            const PathBuffers cur = path_buffers(ws, (int)(k & 1u)), nxt = path_buffers(ws, (int)((k & 1u) ^ 1u));
            if (k > 0) {
                ++n_trace;
                int e = kt.begin(bs);
                launch_trace_closest(bs, tg, ds, cur.rayO, cur.rayD, nullptr, bc, bc + YK_CTRL_HEAD, ws.hit.as<int>(), nullptr, nullptr, ws.spill.as<uint2>(), spill_stride,
                                     error_block(ctx), counters());
                kt.end(e, 0, bs);
            }
            launch_guides_step(bs, scene->dev, cur, nxt, ws.hit.as<int>(), bc, bc + YK_CTRL_STRIDE, n, k, k == rq.max_through, pixel_xy, rq.guides_res_x,
                               reinterpret_cast<float4*>(rq.d_out), reinterpret_cast<uint4*>(rq.d_ids), reinterpret_cast<uint32_t*>(rq.d_through));
        }
        return YK_OK;
    }

    yk_status render_chunk(const yk_plan::Chunk& c) {
        const uint32_t spp = plan.spp;
        HIP_TRY(ctx, ctx->sample_buf.ensure((size_t)c.npx * spp * 16));
        sample_buf = ctx->sample_buf.as<float4>();
        yk_status rc = make_pixel_tables(c);
        if (rc != YK_OK) return rc;
        // the pixel's share of every camera sample's sampler start, once per pixel (yk_rng.h, PixelSampler)
        HIP_TRY(ctx, ctx->pixel_aux.ensure((size_t)c.npx * 16));
        launch_pixel_sampler(st, prm.sampler, pixel_xy, c.npx, ctx->pixel_aux.as<uint4>());
        const bool two = plan.n_ws == 2;
        if (two) {  // the second stream starts after the pixel table exists
            HIP_TRY(ctx, hipEventRecord(ctx->ws[0].done, st));
            HIP_TRY(ctx, hipStreamWaitEvent(ctx->ws[1].stream, ctx->ws[0].done, 0));
        }
        const uint64_t work = (uint64_t)c.npx * spp;
        which = 0;
        ws_busy[0] = ws_busy[1] = false;
        for (uint64_t w0 = 0; w0 < work; w0 += plan.batch) {
            WorkSet& ws = ctx->ws[which];
            if ((rc = gate_on_cancel(ws, w0, work)) != YK_OK) return rc;
            hipStream_t bs = two ? ws.stream : st;
            if ((rc = enqueue_batch(ws, bs, w0, (uint32_t)std::min<uint64_t>(plan.batch, work - w0))) != YK_OK) return rc;
            if (rq.cancel) {
                HIP_TRY(ctx, hipEventRecord(ws.ev_batch, bs));
                ws_busy[which] = true;
            }
            if (two) which ^= 1;
        }
        if (two) {  // resolve (on the caller-visible stream) waits for the second stream
            HIP_TRY(ctx, hipEventRecord(ctx->ws[1].done, ctx->ws[1].stream));
            HIP_TRY(ctx, hipStreamWaitEvent(st, ctx->ws[1].done, 0));
        }
        float* out = reinterpret_cast<float*>(rq.d_out) + 3 * (size_t)c.px0;
        if (rq.guides_res_x)  // k_guides wrote every record at its pixel: nothing to resolve
            ;
        else if (rq.pixels && rq.d_film_sum)  // the fused route: the chunk's samples into the film sums and the statistics
            launch_ad_fold_samples(st, pixel_xy, c.npx, sample_buf, spp, rq.pixels->res_x, reinterpret_cast<float*>(rq.d_film_sum), rq.d_stats);
        else if (plan.accumulating)  // raw values, pass-major over the whole tile list
            launch_resolve_passes(st, sample_buf, c.npx, spp, out, 3 * (size_t)plan.total_px);
        else
            launch_resolve(st, sample_buf, c.npx, spp, out);
        return YK_OK;
    }

    yk_status finish_call() {
        yk_render_stats* stats = rq.stats;
        unsigned words[4];
        if (stats) {
            HIP_TRY(ctx, hipEventRecord(frame_ev.b, st));
            // a synchronous call: the predicate is polled while the GPU works
            if (wait_polling(ctx, frame_ev.b, st, rq.cancel, rq.user)) return fail(ctx, YK_ERR_CANCELLED, "cancelled by early_termination_predicate");
            if (ctx->cancel_raised.load(std::memory_order_acquire)) return fail(ctx, YK_ERR_CANCELLED, "interrupted (yk_context_interrupt)");
            HIP_TRY(ctx, hipGetLastError());
            std::memset(stats, 0, sizeof(*stats));
            unsigned long long host_counters[YK_COUNTER_BYTES / 8];
            HIP_TRY(ctx, hipMemcpy(host_counters, counters(), YK_COUNTER_BYTES, hipMemcpyDeviceToHost));
            std::memcpy(words, host_counters + 16, sizeof(words));
            float ms = 0.0f;
            (void)hipEventElapsedTime(&ms, frame_ev.a, frame_ev.b);
            stats->rays = host_counters[0];
            stats->shadow_rays = host_counters[1];
            stats->samples = plan.total_work;
            stats->seconds_total = ms * 1e-3;
            stats->seconds_trace = kt.total(0);
            stats->seconds_shadow = kt.total(1);
            stats->seconds_shade = kt.total(2);
            stats->trace_launches = n_trace;
            stats->shadow_launches = n_shadow;
            stats->batches = n_batches;
            return error_block_status(ctx, words);
        }
        if (scene->bvh->depth <= 64) return YK_OK;
        // A tree deeper than the reference's 64-entry stack (bvh.rs:172-174) can overflow it: such a render is
        // not left asynchronous — the flag is read before the call returns, whoever the caller is.
        HIP_TRY(ctx, hipMemcpyAsync(words, error_block(ctx), sizeof(words), hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, hipStreamSynchronize(st));
        return error_block_status(ctx, words);
    }
};

static yk_status render_tiles_impl(yk_context* ctx, const RenderRequest& rq) try {
    if (!ctx) return YK_ERR_INVALID_ARGUMENT;
    YK_LOCK(ctx);
    struct HandBack {  // on every exit path: whatever was enqueued is ordered before the caller's next work
        yk_context* c;
        hipStream_t caller;
        ~HandBack() {
            if (!caller) return;
            if (hipEventRecord(c->ev_out, c->stream) == hipSuccess) (void)hipStreamWaitEvent(caller, c->ev_out, 0);
        }
    } hand_back{ctx, nullptr};
    Submission s(ctx, rq);
    yk_status rc = s.check_and_plan();
    if (rc != YK_OK) return rc;
    // The render always runs on the context's own streams; a caller's stream hands over to them
    // and takes over again at the end (two event waits), so the work is ordered on it as if it
    // had been launched there — and the main / side stream pair keeps its own hardware queues.
    if (hipStream_t caller = (hipStream_t)rq.stream) {
        HIP_TRY(ctx, hipEventRecord(ctx->ev_in, caller));
        HIP_TRY(ctx, hipStreamWaitEvent(s.st, ctx->ev_in, 0));
        hand_back.caller = caller;
    }
    if ((rc = s.grow_buffers()) != YK_OK) return rc;
    if ((rc = s.begin_call()) != YK_OK) return rc;
#ifdef YK_EXPERIMENT_GRAPH  // timing builds only (tools/micro/graph_replay_experiment.h)
    YK_GRAPH_BEGIN
#endif
    for (const yk_plan::Chunk& c : s.plan.chunks)
        if ((rc = s.render_chunk(c)) != YK_OK) return rc;
    HIP_TRY(ctx, hipGetLastError());
#ifdef YK_EXPERIMENT_GRAPH
    YK_GRAPH_END
#endif
    return s.finish_call();
} YK_CATCH(ctx)

// a render into a host array: the output staged around the device call
static yk_status render_tiles_host(yk_context* ctx, RenderRequest rq, float* out_rgb) {
    if (!ctx) return YK_ERR_INVALID_ARGUMENT;
    YK_LOCK(ctx);
    if (!rq.tiles || rq.n_tiles == 0 || !out_rgb) return fail(ctx, YK_ERR_INVALID_ARGUMENT, "null argument");
    std::vector<uint32_t> off;
    yk_status st = tile_offsets(ctx, rq.tiles, rq.n_tiles, off, "too many pixels in one call");
    if (st != YK_OK) return st;
    if (rq.n_passes == 0 || rq.n_passes > 0xFFFFu) return fail(ctx, YK_ERR_INVALID_ARGUMENT, "bad number of passes");
    Staging sg(ctx);
    rq.d_out = sg.output(out_rgb, (size_t)off.back() * 3 * rq.n_passes);
    if (!sg.ok()) return sg.status();
    yk_render_stats local;
    if (!rq.stats) rq.stats = &local;
    if ((st = render_tiles_impl(ctx, rq)) != YK_OK) return st;
    return sg.finish();
}

// The guides: the ShadingNormals integrator's trace of the whole film as one tile under a 1 x 1 Stratified sampler without
// jitter, whose camera sample is the pixel centre whatever its seed, so the ray is Camera::ray((x + 0.5, y + 0.5)).
// through != NULL: the pass through glass (yk_guides_through.h) with its bound and its third output.
struct GuidesThrough {
    uint32_t max_through;
    void* d_through;
};
static yk_status render_guides(yk_context* ctx, const yk_scene* scene, const yk_camera* camera, uint16_t res_x, uint16_t res_y, void* d_guides, void* stream, void* d_ids = nullptr,
                               const GuidesThrough* through = nullptr) {
    yk_sampler_desc smp = {};
    smp.kind = YK_SAMPLER_STRATIFIED;
    smp.nx = smp.ny = 1;
    yk_integrator_desc integ = {};
    integ.kind = YK_INTEGRATOR_SHADING_NORMALS;
    const yk_tile film = {0, 0, res_x, res_y};
    RenderRequest rq;
    rq.scene = scene;
    rq.camera = camera;
    rq.sampler = &smp;
    rq.integrator = &integ;
    rq.tiles = &film;
    rq.n_tiles = 1;
    rq.d_out = d_guides;
    rq.guides_res_x = res_x;
    rq.d_ids = d_ids;
    if (through) {
        rq.through = true;
        rq.max_through = through->max_through;
        rq.d_through = through->d_through;
    }
    rq.stream = stream;
    return render_tiles_impl(ctx, rq);
}

static yk_status film_update_list(yk_context* ctx, const yk_tile_list* list, const void* d_tile_rgb, uint16_t res_x, uint16_t res_y, void* d_film_rgb,
                                  void* stream, int accumulate, uint32_t n_passes) {
    if (!ctx) return YK_ERR_INVALID_ARGUMENT;
    YK_LOCK(ctx);
    if (!list || !d_tile_rgb || !d_film_rgb) return fail(ctx, YK_ERR_INVALID_ARGUMENT, "null argument");
    if (list->device != ctx->device) return fail(ctx, YK_ERR_INVALID_ARGUMENT, "tile list was not created on this context's device");
    for (const yk_tile& t : list->tiles)
        if (t.x1 > res_x || t.y1 > res_y) return fail(ctx, YK_ERR_INVALID_ARGUMENT, "update_tile: Tile doesn't fit film");
    (void)hipSetDevice(ctx->device);
    hipStream_t st = stream ? (hipStream_t)stream : ctx->stream;
    if (n_passes == 0 || n_passes > 0xFFFFu) return fail(ctx, YK_ERR_INVALID_ARGUMENT, "bad number of passes");
    launch_film_scatter(st, list->pixel_xy.as<uint32_t>(), list->off.back(), reinterpret_cast<const float*>(d_tile_rgb), res_x,
                        reinterpret_cast<float*>(d_film_rgb), accumulate ? 1 : 0, n_passes, 3 * (size_t)list->off.back());
    HIP_TRY(ctx, hipGetLastError());
    return YK_OK;  // asynchronous: ordered on `stream`
}

static yk_status film_tiles_device(yk_context* ctx, const yk_tile* tiles, size_t n_tiles, const void* d_tile_rgb, uint16_t res_x, uint16_t res_y,
                                   void* d_film_rgb, void* stream, int accumulate) try {
    if (!ctx) return YK_ERR_INVALID_ARGUMENT;
    YK_LOCK(ctx);
    if (!tiles || !d_tile_rgb || !d_film_rgb || n_tiles == 0) return fail(ctx, YK_ERR_INVALID_ARGUMENT, "null argument");
    (void)hipSetDevice(ctx->device);
    hipStream_t st = stream ? (hipStream_t)stream : ctx->stream;
    std::vector<uint32_t> off;
    const yk_plan::TileRefusal no = yk_plan::tile_ranges(tiles, n_tiles, off, res_x, res_y);
    if (no == yk_plan::TILES_TOO_MANY_PIXELS) return fail(ctx, YK_ERR_INVALID_ARGUMENT, "too many pixels");
    if (no != yk_plan::TILES_OK) return fail(ctx, YK_ERR_INVALID_ARGUMENT, "update_tile: Tile doesn't fit film");
    const uint32_t total = off.back();
    HIP_TRY(ctx, ctx->film_tiles.ensure(n_tiles * sizeof(yk_tile)));
    HIP_TRY(ctx, ctx->film_tile_off.ensure((n_tiles + 1) * 4));
    HIP_TRY(ctx, ctx->film_pixel_xy.ensure((size_t)total * 4));
    HIP_TRY(ctx, hipMemcpyAsync(ctx->film_tiles.p, tiles, n_tiles * sizeof(yk_tile), hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemcpyAsync(ctx->film_tile_off.p, off.data(), off.size() * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    launch_pixel_table(st, ctx->film_tiles.as<yk_tile>(), ctx->film_tile_off.as<uint32_t>(), (uint32_t)n_tiles, total, ctx->film_pixel_xy.as<uint32_t>());
    launch_film_scatter(st, ctx->film_pixel_xy.as<uint32_t>(), total, reinterpret_cast<const float*>(d_tile_rgb), res_x, reinterpret_cast<float*>(d_film_rgb), accumulate);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipStreamSynchronize(st));
    return YK_OK;
} YK_CATCH(ctx)

// ------------------------------------------------------------------ yk_li / yk_li_debug: what both do
// One ray per table entry (pixel, sample index), generated by launch_raygen_user into work set 0.
struct LiCall {
    yk_context* const ctx;
    const yk_scene* const scene;
    const size_t n;
    RenderParams prm;
    const uint32_t* d_sample_index = nullptr;
    unsigned words[4];  // the error block, read back

    // The checks and the parameters.  `refuse_size`, `refuse_integrator`: the entry point's own refusals (NULL: none), said
    // where they have always been said.
    yk_status check(bool arrays_given, const yk_sampler_desc* sampler, const yk_integrator_desc* integrator, const uint32_t* sample_index, const char* refuse_size,
                    const char* refuse_integrator) {
        if (!scene || !arrays_given || n == 0) return fail(ctx, YK_ERR_INVALID_ARGUMENT, "null argument");
        if (yk_status rs = scene_on_context(ctx, scene, "")) return rs;
        if (n > ((size_t)1 << 28)) return fail(ctx, YK_ERR_INVALID_ARGUMENT, "too many rays");
        if (refuse_size) return fail(ctx, YK_ERR_INVALID_ARGUMENT, refuse_size);
        yk_status ps = make_params(ctx, sampler, integrator, prm);
        if (ps != YK_OK) return ps;
        if (refuse_integrator) return fail(ctx, YK_ERR_UNSUPPORTED, refuse_integrator);
        prm.spe = 1;  // one table entry (pixel, sample index) per ray
        for (size_t i = 0; i < n; ++i)
            if (sample_index[i] >= prm.sampler.spp) return fail(ctx, YK_ERR_INVALID_ARGUMENT, "sample_index >= samples per pixel");
        return YK_OK;
    }
    // the buffers of work set 0 and the context's counters: cancel_ref(ctx) points into them, so it is taken after this
    yk_status grow() {
        yk_status wb = ensure_work_buffers(ctx, ctx->ws[0], n, scene->n_lights, scene->n_delta_lights);
        if (wb != YK_OK) return wb;
        if ((wb = ensure_spill(ctx, ctx->ws[0])) != YK_OK) return wb;
        HIP_TRY(ctx, ctx->pixel_xy.ensure(n * 4));
        HIP_TRY(ctx, ctx->sample_buf.ensure(n * 16));
        return YK_OK;
    }
    // the four inputs staged, counters and control block zeroed, the rays generated
    yk_status raygen(Staging& sg, const float* ray_o, const float* ray_d, const uint16_t* pixel_xy, const uint32_t* sample_index, uint32_t dimension) {
        const float* d_ray_o = sg.upload(ray_o, n * 3);
        const float* d_ray_d = sg.upload(ray_d, n * 3);
        const uint16_t* d_pixel_xy = sg.upload(pixel_xy, n * 2);
        d_sample_index = sg.upload(sample_index, n);
        if (!sg.ok()) return sg.status();
        unsigned* ctrl = ctx->ws[0].ctrl.as<unsigned>();
        HIP_TRY(ctx, hipMemsetAsync(ctx->counters.p, 0, YK_COUNTER_BYTES, sg.stream));  // the error block with it: stack-overflow flag, interruption word
        HIP_TRY(ctx, hipMemsetAsync(ctrl, 0, YK_CTRL_WORDS * 4, sg.stream));
        launch_raygen_user(sg.stream, prm, d_ray_o, d_ray_d, d_pixel_xy, d_sample_index, dimension, (uint32_t)n, path_buffers(ctx->ws[0], 0), ctx->sample_buf.as<float4>(),
                           ctx->pixel_xy.as<uint32_t>(), ctrl + YK_CTRL_BOUNCE(0));
        return YK_OK;
    }
    // after the synchronisation: the verdict of the error block, then the float4 samples as RGB
    yk_status verdict_and_rgb(const std::vector<float>& rgba, float* out_li) {
        yk_status st = error_block_status(ctx, words);
        for (size_t i = 0; st == YK_OK && i < n; ++i) std::memcpy(out_li + 3 * i, rgba.data() + 4 * i, 12);
        return st;
    }
};

extern "C" {

yk_status yk_render_tiles_device(yk_context* ctx, const yk_scene* scene, const yk_camera* camera, const yk_sampler_desc* sampler,
                                 const yk_integrator_desc* integrator, const yk_tile* tiles, size_t n_tiles, void* d_out_rgb, void* stream,
                                 yk_render_stats* stats, yk_cancel_fn cancel, void* user) {
    RenderRequest rq = request_for(scene, camera, sampler, integrator, d_out_rgb, stream, stats, cancel, user);
    rq.tiles = tiles;
    rq.n_tiles = n_tiles;
    return render_tiles_impl(ctx, rq);
}

yk_status yk_render_tiles_accumulating_device(yk_context* ctx, const yk_scene* scene, const yk_camera* camera, const yk_sampler_desc* sampler,
                                              const yk_integrator_desc* integrator, const yk_tile* tiles, const uint16_t* tile_samples, size_t n_tiles,
                                              void* d_out_rgb, void* stream, yk_render_stats* stats, yk_cancel_fn cancel, void* user) {
    if (!ctx) return YK_ERR_INVALID_ARGUMENT;
    YK_LOCK(ctx);
    if (!tile_samples) return fail(ctx, YK_ERR_INVALID_ARGUMENT, "null tile_samples");
    RenderRequest rq = request_for(scene, camera, sampler, integrator, d_out_rgb, stream, stats, cancel, user);
    rq.tiles = tiles;
    rq.tile_samples = tile_samples;
    rq.n_tiles = n_tiles;
    return render_tiles_impl(ctx, rq);
}

yk_status yk_render_tiles_accumulating_passes(yk_context* ctx, const yk_scene* scene, const yk_camera* camera, const yk_sampler_desc* sampler,
                                              const yk_integrator_desc* integrator, const yk_tile* tiles, const uint16_t* tile_samples, size_t n_tiles,
                                              uint32_t n_passes, float* out_rgb, yk_render_stats* stats, yk_cancel_fn cancel, void* user) {
    if (!ctx) return YK_ERR_INVALID_ARGUMENT;
    YK_LOCK(ctx);
    if (!tile_samples) return fail(ctx, YK_ERR_INVALID_ARGUMENT, "null tile_samples");
    RenderRequest rq = request_for(scene, camera, sampler, integrator, nullptr, nullptr, stats, cancel, user);  // the output is staged
    rq.tiles = tiles;
    rq.tile_samples = tile_samples;
    rq.n_tiles = n_tiles;
    rq.n_passes = n_passes;
    return render_tiles_host(ctx, rq, out_rgb);
}

yk_status yk_render_tiles_accumulating(yk_context* ctx, const yk_scene* scene, const yk_camera* camera, const yk_sampler_desc* sampler,
                                       const yk_integrator_desc* integrator, const yk_tile* tiles, const uint16_t* tile_samples, size_t n_tiles,
                                       float* out_rgb, yk_render_stats* stats, yk_cancel_fn cancel, void* user) {
    return yk_render_tiles_accumulating_passes(ctx, scene, camera, sampler, integrator, tiles, tile_samples, n_tiles, 1, out_rgb, stats, cancel, user);
}

yk_status yk_render_tiles(yk_context* ctx, const yk_scene* scene, const yk_camera* camera, const yk_sampler_desc* sampler,
                          const yk_integrator_desc* integrator, const yk_tile* tiles, size_t n_tiles, float* out_rgb, yk_render_stats* stats,
                          yk_cancel_fn cancel, void* user) {
    RenderRequest rq = request_for(scene, camera, sampler, integrator, nullptr, nullptr, stats, cancel, user);  // the output is staged
    rq.tiles = tiles;
    rq.n_tiles = n_tiles;
    return render_tiles_host(ctx, rq, out_rgb);
}

yk_status yk_render_tile(yk_context* ctx, const yk_scene* scene, const yk_camera* camera, const yk_sampler_desc* sampler,
                         const yk_integrator_desc* integrator, const yk_tile* tile, float* tile_pixels, uint64_t* out_rays) {
    yk_render_stats stats;
    yk_status st = yk_render_tiles(ctx, scene, camera, sampler, integrator, tile, 1, tile_pixels, &stats, nullptr, nullptr);
    if (st == YK_OK && out_rays) *out_rays = stats.rays;
    return st;
}

yk_status yk_tile_list_create(yk_context* ctx, const yk_tile* tiles, const uint16_t* tile_samples, size_t n_tiles, yk_tile_list** out) try {
    if (!ctx) return YK_ERR_INVALID_ARGUMENT;
    YK_LOCK(ctx);
    if (!tiles || !out || n_tiles == 0) return fail(ctx, YK_ERR_INVALID_ARGUMENT, "null argument");
    *out = nullptr;
    std::unique_ptr<yk_tile_list> l(new yk_tile_list());
    l->device = ctx->device;
    l->tiles.assign(tiles, tiles + n_tiles);
    if (tile_samples) l->samples.assign(tile_samples, tile_samples + n_tiles);
    yk_status rc = tile_offsets(ctx, tiles, n_tiles, l->off, "too many pixels in one list");
    if (rc != YK_OK) return rc;
    const uint32_t total = l->off.back();
    (void)hipSetDevice(ctx->device);
    hipStream_t st = ctx->stream;
    auto tryhip = [&](hipError_t e, const char* what) {
        if (e != hipSuccess && rc == YK_OK) rc = fail(ctx, e == hipErrorOutOfMemory ? YK_ERR_OUT_OF_MEMORY : YK_ERR_DEVICE, std::string(what) + ": " + hipGetErrorString(e));
    };
    tryhip(ctx->tiles.ensure(n_tiles * sizeof(yk_tile)), "tiles");
    tryhip(ctx->tile_off.ensure((n_tiles + 1) * 4), "tile offsets");
    tryhip(l->pixel_xy.ensure((size_t)total * 4), "pixel table");
    if (tile_samples) {
        tryhip(ctx->tile_sample.ensure(n_tiles * 2), "tile samples");
        tryhip(l->pixel_sample.ensure((size_t)total * 4), "pixel samples");
    }
    if (rc == YK_OK) {
        tryhip(hipMemcpyAsync(ctx->tiles.p, tiles, n_tiles * sizeof(yk_tile), hipMemcpyHostToDevice, st), "upload tiles");
        tryhip(hipMemcpyAsync(ctx->tile_off.p, l->off.data(), l->off.size() * 4, hipMemcpyHostToDevice, st), "upload offsets");
        if (tile_samples) tryhip(hipMemcpyAsync(ctx->tile_sample.p, tile_samples, n_tiles * 2, hipMemcpyHostToDevice, st), "upload samples");
    }
    if (rc == YK_OK) {
        launch_pixel_table(st, ctx->tiles.as<yk_tile>(), ctx->tile_off.as<uint32_t>(), (uint32_t)n_tiles, total, l->pixel_xy.as<uint32_t>(),
                           tile_samples ? ctx->tile_sample.as<uint16_t>() : nullptr, tile_samples ? l->pixel_sample.as<uint32_t>() : nullptr);
        tryhip(hipGetLastError(), "pixel table kernel");
        tryhip(hipStreamSynchronize(st), "sync");
    }
    if (rc != YK_OK) {
        l->pixel_xy.release();
        l->pixel_sample.release();
        return rc;
    }
    *out = l.release();
    return YK_OK;
} YK_CATCH(ctx)

void yk_tile_list_destroy(yk_tile_list* l) {
    if (!l) return;
    if (l->device >= 0) (void)hipSetDevice(l->device);
    l->pixel_xy.release();
    l->pixel_sample.release();
    delete l;
}

// a prepared list: plain, with the passes of an accumulating list, or with a first sample index for every tile of a plain one
static yk_status render_tile_list(yk_context* ctx, RenderRequest rq, const yk_tile_list* list, const char* wrong_list) {
    if (!ctx) return YK_ERR_INVALID_ARGUMENT;
    if (!list) return fail(ctx, YK_ERR_INVALID_ARGUMENT, "null tile list");
    if (wrong_list) return fail(ctx, YK_ERR_INVALID_ARGUMENT, wrong_list);
    rq.list = list;
    return render_tiles_impl(ctx, rq);
}

yk_status yk_render_tile_list_device(yk_context* ctx, const yk_scene* scene, const yk_camera* camera, const yk_sampler_desc* sampler,
                                     const yk_integrator_desc* integrator, const yk_tile_list* list, void* d_out_rgb, void* stream,
                                     yk_render_stats* stats, yk_cancel_fn cancel, void* user) {
    return render_tile_list(ctx, request_for(scene, camera, sampler, integrator, d_out_rgb, stream, stats, cancel, user), list, nullptr);
}

yk_status yk_render_tile_list_passes_device(yk_context* ctx, const yk_scene* scene, const yk_camera* camera, const yk_sampler_desc* sampler,
                                            const yk_integrator_desc* integrator, const yk_tile_list* list, uint32_t n_passes, void* d_out_rgb, void* stream,
                                            yk_render_stats* stats, yk_cancel_fn cancel, void* user) {
    RenderRequest rq = request_for(scene, camera, sampler, integrator, d_out_rgb, stream, stats, cancel, user);
    rq.n_passes = n_passes;
    return render_tile_list(ctx, rq, list, list && list->samples.empty() ? "passes need an accumulating tile list (tile_samples)" : nullptr);
}

yk_status yk_render_tile_list_samples_device(yk_context* ctx, const yk_scene* scene, const yk_camera* camera, const yk_sampler_desc* sampler,
                                             const yk_integrator_desc* integrator, const yk_tile_list* list, uint32_t first_sample, uint32_t n_passes,
                                             void* d_out_rgb, void* stream, yk_render_stats* stats, yk_cancel_fn cancel, void* user) {
    RenderRequest rq = request_for(scene, camera, sampler, integrator, d_out_rgb, stream, stats, cancel, user);
    rq.n_passes = n_passes;
    rq.uniform_first_sample = (int64_t)first_sample;
    return render_tile_list(ctx, rq, list, list && !list->samples.empty() ? "the list carries per-tile sample indices: use yk_render_tile_list_passes_device" : nullptr);
}

// a pixel list into a pass-major buffer, or (d_film_sum, d_stats) fused into a film; an empty list launches nothing
static yk_status render_pixel_list(yk_context* ctx, RenderRequest rq, const yk_pixel_list* list, const char* who) {
    if (!list) return fail(ctx, YK_ERR_INVALID_ARGUMENT, std::string(who) + ": null pixel list");
    rq.pixels = list;
    if (list->n == 0) {  // the arguments are still checked; the plan has no chunk and nothing is enqueued
        Submission s(ctx, rq);
        yk_status rc = s.check_and_plan();
        if (rc == YK_OK && rq.stats) std::memset(rq.stats, 0, sizeof(*rq.stats));
        return rc;
    }
    return render_tiles_impl(ctx, rq);
}

yk_status yk_render_pixel_list_device(yk_context* ctx, const yk_scene* scene, const yk_camera* camera, const yk_sampler_desc* sampler, const yk_integrator_desc* integrator,
                                      const yk_pixel_list* list, uint32_t n_passes, void* d_out_rgb, void* stream, yk_render_stats* stats, yk_cancel_fn cancel, void* user) {
    if (!ctx) return YK_ERR_INVALID_ARGUMENT;
    YK_LOCK(ctx);
    if (!d_out_rgb || misaligned(4, d_out_rgb)) return fail(ctx, YK_ERR_INVALID_ARGUMENT, "yk_render_pixel_list_device: the output must be given and 4-byte aligned");
    RenderRequest rq = request_for(scene, camera, sampler, integrator, d_out_rgb, stream, stats, cancel, user);
    rq.n_passes = n_passes;
    return render_pixel_list(ctx, rq, list, "yk_render_pixel_list_device");
}

// select -> stop on an empty selection or at max_rounds -> the fused render of the list with round_passes -> again
yk_status yk_render_adaptive_device(yk_context* ctx, const yk_scene* scene, const yk_camera* camera, const yk_sampler_desc* sampler, const yk_integrator_desc* integrator,
                                    const yk_adaptive_desc* desc, uint16_t res_x, uint16_t res_y, void* d_film_sum, void* d_stats, void* stream, yk_adaptive_info* info,
                                    yk_cancel_fn cancel, void* user) {
    if (!ctx) return YK_ERR_INVALID_ARGUMENT;
    YK_LOCK(ctx);
    if (info) std::memset(info, 0, sizeof(*info));
    if (!ad_desc_ok(desc) || !scene || !camera || !d_film_sum || !d_stats || res_x == 0 || res_y == 0) return fail(ctx, YK_ERR_INVALID_ARGUMENT, "yk_render_adaptive_device: bad argument");
    const size_t n_px = (size_t)res_x * res_y;
    if (misaligned(4, d_film_sum) || misaligned(16, d_stats)) return fail(ctx, YK_ERR_INVALID_ARGUMENT, "yk_render_adaptive_device: film must be 4-byte aligned, statistics 16-byte aligned");
    if (overlaps(d_film_sum, n_px * 12, d_stats, n_px * 16)) return fail(ctx, YK_ERR_INVALID_ARGUMENT, "yk_render_adaptive_device: film and statistics overlap");
    RenderParams prm;  // the sampler and the integrator are refused before the first selection, not after it
    yk_status rc = make_params(ctx, sampler, integrator, prm);
    if (rc != YK_OK) return rc;
    if (desc->max_samples > prm.sampler.spp) return fail(ctx, YK_ERR_INVALID_ARGUMENT, "yk_render_adaptive_device: max_samples beyond the sampler's samples per pixel");
    yk_pixel_list* made = nullptr;
    if ((rc = yk_pixel_list_create(ctx, res_x, res_y, &made)) != YK_OK) return rc;
    std::unique_ptr<yk_pixel_list, void (*)(yk_pixel_list*)> list(made, yk_pixel_list_destroy);
    yk_adaptive_info got = {};
    hipStream_t st = device_call_stream(ctx, stream);
    for (;;) {
        uint32_t n = 0;
        if ((rc = adaptive_select_into(ctx, st, desc, d_stats, list.get(), &n)) != YK_OK) return rc;
        if (n == 0) {
            got.converged = 1;
            break;
        }
        if (desc->max_rounds && got.rounds == desc->max_rounds) break;
        yk_render_stats stats;
        RenderRequest rq = request_for(scene, camera, sampler, integrator, nullptr, stream, &stats, cancel, user);
        rq.n_passes = desc->round_passes;
        rq.d_film_sum = d_film_sum;
        rq.d_stats = d_stats;
        if ((rc = render_pixel_list(ctx, rq, list.get(), "yk_render_adaptive_device")) != YK_OK) return rc;
        if (got.rounds == 0) got.first_pixels = n;
        got.last_pixels = n;
        ++got.rounds;
        got.samples += stats.samples;
        got.rays += stats.rays;
        got.shadow_rays += stats.shadow_rays;
        if (info) *info = got;
    }
    if (info) *info = got;
    return YK_OK;
}

// An interruption from any thread (the call that renders holds the context's lock for its whole duration, this one
// takes none): what the context has enqueued stops at the kernels' next look at the word, the next submission waits
// for it to drain and clears the word.
yk_status yk_context_interrupt(yk_context* ctx) {
    if (!ctx) return YK_ERR_INVALID_ARGUMENT;
    raise_cancel(ctx, false);  // the host word only: no HIP call from a thread that may not have the device current
    return YK_OK;
}

yk_status yk_film_accumulate_tile_list_passes_device(yk_context* ctx, const yk_tile_list* list, const void* d_passes_rgb, uint32_t n_passes, uint16_t res_x,
                                                     uint16_t res_y, void* d_film_rgb, void* stream) {
    return film_update_list(ctx, list, d_passes_rgb, res_x, res_y, d_film_rgb, stream, 1, n_passes);
}

yk_status yk_film_update_tile_list_device(yk_context* ctx, const yk_tile_list* list, const void* d_tile_rgb, uint16_t res_x, uint16_t res_y,
                                          void* d_film_rgb, void* stream, int accumulate) {
    return film_update_list(ctx, list, d_tile_rgb, res_x, res_y, d_film_rgb, stream, accumulate, 1);
}

yk_status yk_film_update_tiles_device(yk_context* ctx, const yk_tile* tiles, size_t n_tiles, const void* d_tile_rgb, uint16_t res_x, uint16_t res_y,
                                      void* d_film_rgb, void* stream) {
    return film_tiles_device(ctx, tiles, n_tiles, d_tile_rgb, res_x, res_y, d_film_rgb, stream, 0);
}

yk_status yk_film_accumulate_tiles_device(yk_context* ctx, const yk_tile* tiles, size_t n_tiles, const void* d_tile_rgb, uint16_t res_x, uint16_t res_y,
                                          void* d_film_rgb, void* stream) {
    return film_tiles_device(ctx, tiles, n_tiles, d_tile_rgb, res_x, res_y, d_film_rgb, stream, 1);
}

yk_status yk_render_guides_device(yk_context* ctx, const yk_scene* scene, const yk_camera* camera, uint16_t res_x, uint16_t res_y, void* d_guides, void* stream) {
    if (!ctx) return YK_ERR_INVALID_ARGUMENT;
    YK_LOCK(ctx);
    if (!scene || !camera || !d_guides || res_x == 0 || res_y == 0) return fail(ctx, YK_ERR_INVALID_ARGUMENT, "yk_render_guides_device: bad argument");
    if (misaligned(16, d_guides)) return fail(ctx, YK_ERR_INVALID_ARGUMENT, "yk_render_guides_device: guides must be 16-byte aligned");
    return render_guides(ctx, scene, camera, res_x, res_y, d_guides, stream);
}

yk_status yk_render_guides(yk_context* ctx, const yk_scene* scene, const yk_camera* camera, uint16_t res_x, uint16_t res_y, yk_guide* out) {
    if (!ctx) return YK_ERR_INVALID_ARGUMENT;
    YK_LOCK(ctx);
    if (!scene || !camera || !out || res_x == 0 || res_y == 0) return fail(ctx, YK_ERR_INVALID_ARGUMENT, "yk_render_guides: bad argument");
    Staging sg(ctx);
    yk_guide* d_guides = sg.output(out, (size_t)res_x * res_y);
    return sg.run([&] { return render_guides(ctx, scene, camera, res_x, res_y, d_guides, nullptr); });
}

// The guides with the surface ids beside them (yk_motion.h): the same single trace, k_guides_ids instead of k_guides.
yk_status yk_render_guides_ids_device(yk_context* ctx, const yk_scene* scene, const yk_camera* camera, uint16_t res_x, uint16_t res_y, void* d_guides, void* d_ids, void* stream) {
    if (!ctx) return YK_ERR_INVALID_ARGUMENT;
    YK_LOCK(ctx);
    if (!scene || !camera || (!d_guides && !d_ids) || res_x == 0 || res_y == 0) return fail(ctx, YK_ERR_INVALID_ARGUMENT, "yk_render_guides_ids_device: bad argument");
    if (misaligned(16, d_guides, d_ids)) return fail(ctx, YK_ERR_INVALID_ARGUMENT, "yk_render_guides_ids_device: guides and ids must be 16-byte aligned");
    const size_t n_px = (size_t)res_x * res_y;
    if (d_guides && d_ids && overlaps(d_guides, n_px * sizeof(yk_guide), d_ids, n_px * sizeof(yk_surface_id)))
        return fail(ctx, YK_ERR_INVALID_ARGUMENT, "yk_render_guides_ids_device: guides and ids overlap");
    return render_guides(ctx, scene, camera, res_x, res_y, d_guides, stream, d_ids);  // without ids: yk_render_guides_device
}

yk_status yk_render_guides_ids(yk_context* ctx, const yk_scene* scene, const yk_camera* camera, uint16_t res_x, uint16_t res_y, yk_guide* out_guides, yk_surface_id* out_ids) {
    if (!ctx) return YK_ERR_INVALID_ARGUMENT;
    YK_LOCK(ctx);
    if (!scene || !camera || (!out_guides && !out_ids) || res_x == 0 || res_y == 0) return fail(ctx, YK_ERR_INVALID_ARGUMENT, "yk_render_guides_ids: bad argument");
    const size_t n_px = (size_t)res_x * res_y;
    Staging sg(ctx);
    yk_guide* d_guides = sg.output(out_guides, n_px);  // either may be left out
    yk_surface_id* d_ids = sg.output(out_ids, n_px);
    return sg.run([&] { return render_guides(ctx, scene, camera, res_x, res_y, d_guides, nullptr, d_ids); });
}

// The guides through glass (yk_guides_through.h): the records of the surface a pixel shows.  The refusals are
// yk_render_guides_ids_device's, plus the bound on max_through and outputs that overlap one another; nothing is launched
// before the last of them.
yk_status yk_render_guides_through_device(yk_context* ctx, const yk_scene* scene, const yk_camera* camera, uint16_t res_x, uint16_t res_y, uint32_t max_through, void* d_guides,
                                          void* d_ids, void* d_through, void* stream) {
    if (!ctx) return YK_ERR_INVALID_ARGUMENT;
    YK_LOCK(ctx);
    if (!scene || !camera || (!d_guides && !d_ids && !d_through) || res_x == 0 || res_y == 0)
        return fail(ctx, YK_ERR_INVALID_ARGUMENT, "yk_render_guides_through_device: bad argument");
    if (max_through > YK_GUIDES_THROUGH_MAX) return fail(ctx, YK_ERR_INVALID_ARGUMENT, "yk_render_guides_through_device: max_through above YK_GUIDES_THROUGH_MAX");
    if (misaligned(16, d_guides, d_ids)) return fail(ctx, YK_ERR_INVALID_ARGUMENT, "yk_render_guides_through_device: guides and ids must be 16-byte aligned");
    if (misaligned(4, d_through)) return fail(ctx, YK_ERR_INVALID_ARGUMENT, "yk_render_guides_through_device: through must be 4-byte aligned");
    const size_t n_px = (size_t)res_x * res_y;
    const size_t bg = n_px * sizeof(yk_guide), bi = n_px * sizeof(yk_surface_id), bt = n_px * sizeof(uint32_t);
    if ((d_guides && d_ids && overlaps(d_guides, bg, d_ids, bi)) || (d_guides && d_through && overlaps(d_guides, bg, d_through, bt)) ||
        (d_ids && d_through && overlaps(d_ids, bi, d_through, bt)))
        return fail(ctx, YK_ERR_INVALID_ARGUMENT, "yk_render_guides_through_device: outputs overlap");
    const GuidesThrough gt{max_through, d_through};
    return render_guides(ctx, scene, camera, res_x, res_y, d_guides, stream, d_ids, &gt);
}

yk_status yk_render_guides_through(yk_context* ctx, const yk_scene* scene, const yk_camera* camera, uint16_t res_x, uint16_t res_y, uint32_t max_through, yk_guide* out_guides,
                                   yk_surface_id* out_ids, uint32_t* out_through) {
    if (!ctx) return YK_ERR_INVALID_ARGUMENT;
    YK_LOCK(ctx);
    if (!scene || !camera || (!out_guides && !out_ids && !out_through) || res_x == 0 || res_y == 0) return fail(ctx, YK_ERR_INVALID_ARGUMENT, "yk_render_guides_through: bad argument");
    if (max_through > YK_GUIDES_THROUGH_MAX) return fail(ctx, YK_ERR_INVALID_ARGUMENT, "yk_render_guides_through: max_through above YK_GUIDES_THROUGH_MAX");
    const size_t n_px = (size_t)res_x * res_y;
    Staging sg(ctx);
    yk_guide* d_guides = sg.output(out_guides, n_px);  // each may be left out
    yk_surface_id* d_ids = sg.output(out_ids, n_px);
    uint32_t* d_through = sg.output(out_through, n_px);
    const GuidesThrough gt{max_through, d_through};
    return sg.run([&] { return render_guides(ctx, scene, camera, res_x, res_y, d_guides, nullptr, d_ids, &gt); });
}

// The fused pixel-mean albedo (yk_albedo.h): the large film is traced in bands of output rows, so that it never exists as a
// whole — at 1080p with s = 4 its ids alone are 530 MB.  A band is render_guides' request for the rows [s*y0, s*(y0 + r)) of
// the large film as one tile, its ids written by k_ids_band into the context's band scratch, then k_albedo_mean over the
// band into rows [y0, y0 + r) of the output.  Band after band in the caller's stream order: the trace hands over from and
// back to `stream` (render_tiles_impl), the reduction runs on it, and the next band's trace waits for it before it writes
// the scratch again.  The scratch is YK_ALBEDO_MEAN_SCRATCH bytes from the first call on; the default band fits it whatever
// the film (a row of ids is at most 65535 * 8 * 16 bytes), so only a larger "albedo_mean_band_rows" ever grows it.
static yk_status render_albedo_mean(yk_context* ctx, const yk_scene* scene, const yk_camera* camera_ss, uint16_t res_x, uint16_t res_y, uint32_t s, void* d_out, void* stream) {
    const uint32_t wide = s * res_x;
    const size_t row_bytes = (size_t)wide * s * sizeof(yk_surface_id);  // the ids under one output row
    uint32_t rows = ctx->albedo_mean.band_rows ? (uint32_t)ctx->albedo_mean.band_rows : (uint32_t)std::max<size_t>(1, YK_ALBEDO_MEAN_SCRATCH / row_bytes);
    rows = std::min<uint32_t>(rows, res_y);
    (void)hipSetDevice(ctx->device);
    HIP_TRY(ctx, ctx->albedo_mean.ids_band.ensure(std::max<size_t>(YK_ALBEDO_MEAN_SCRATCH, rows * row_bytes)));
    const hipStream_t st = device_call_stream(ctx, stream);
    yk_sampler_desc smp = {};
    smp.kind = YK_SAMPLER_STRATIFIED;
    smp.nx = smp.ny = 1;
    yk_integrator_desc integ = {};
    integ.kind = YK_INTEGRATOR_SHADING_NORMALS;
    for (uint32_t y0 = 0; y0 < res_y; y0 += rows) {
        const uint32_t r = std::min<uint32_t>(rows, res_y - y0);
        const yk_tile band = {0, (uint16_t)(s * y0), (uint16_t)wide, (uint16_t)(s * (y0 + r))};
        RenderRequest rq;
        rq.scene = scene;
        rq.camera = camera_ss;
        rq.sampler = &smp;
        rq.integrator = &integ;
        rq.tiles = &band;
        rq.n_tiles = 1;
        rq.guides_res_x = wide;
        rq.d_ids = ctx->albedo_mean.ids_band.p;
        rq.ids_row0 = s * y0;
        rq.ids_band_rows = s * r;
        rq.stream = stream;
        yk_status rc = render_tiles_impl(ctx, rq);
        if (rc != YK_OK) return rc;
        if ((rc = albedo_mean_enqueue(ctx, st, scene, ctx->albedo_mean.ids_band.p, res_x, r, s, reinterpret_cast<yk_albedo*>(d_out) + (size_t)y0 * res_x)) != YK_OK) return rc;
    }
    return YK_OK;
}

static bool albedo_mean_args_ok(const yk_scene* scene, const yk_camera* camera_ss, uint16_t res_x, uint16_t res_y, uint32_t s, const void* out) {
    return scene && camera_ss && out && res_x != 0 && res_y != 0 && s >= 1u && s <= YK_ALBEDO_MEAN_MAX_S && s * res_x <= 65535u && s * res_y <= 65535u;
}

yk_status yk_render_albedo_mean_device(yk_context* ctx, const yk_scene* scene, const yk_camera* camera_ss, uint16_t res_x, uint16_t res_y, uint32_t s, void* d_out, void* stream) try {
    if (!ctx) return YK_ERR_INVALID_ARGUMENT;
    YK_LOCK(ctx);
    if (!albedo_mean_args_ok(scene, camera_ss, res_x, res_y, s, d_out)) return fail(ctx, YK_ERR_INVALID_ARGUMENT, "yk_render_albedo_mean_device: bad argument");
    if (yk_status rs = scene_on_context(ctx, scene, "yk_render_albedo_mean_device")) return rs;
    if (misaligned(16, d_out)) return fail(ctx, YK_ERR_INVALID_ARGUMENT, "yk_render_albedo_mean_device: the output must be 16-byte aligned");
    return render_albedo_mean(ctx, scene, camera_ss, res_x, res_y, s, d_out, stream);
}
YK_CATCH(ctx)

yk_status yk_render_albedo_mean(yk_context* ctx, const yk_scene* scene, const yk_camera* camera_ss, uint16_t res_x, uint16_t res_y, uint32_t s, yk_albedo* out) try {
    if (!ctx) return YK_ERR_INVALID_ARGUMENT;
    YK_LOCK(ctx);
    if (!albedo_mean_args_ok(scene, camera_ss, res_x, res_y, s, out)) return fail(ctx, YK_ERR_INVALID_ARGUMENT, "yk_render_albedo_mean: bad argument");
    if (yk_status rs = scene_on_context(ctx, scene, "yk_render_albedo_mean")) return rs;
    Staging sg(ctx);
    yk_albedo* d_out = sg.output(out, (size_t)res_x * res_y);
    return sg.run([&] { return render_albedo_mean(ctx, scene, camera_ss, res_x, res_y, s, d_out, nullptr); });
}
YK_CATCH(ctx)

yk_status yk_li(yk_context* ctx, const yk_scene* scene, const yk_sampler_desc* sampler, const yk_integrator_desc* integrator, size_t n,
                const float* ray_o, const float* ray_d, const uint16_t* pixel_xy, const uint32_t* sample_index, uint32_t dimension, float* out_li,
                uint32_t* out_ray_counts) try {
    if (!ctx) return YK_ERR_INVALID_ARGUMENT;
    YK_LOCK(ctx);
    LiCall li{ctx, scene, n};
    const bool accepted = integrator && (integrator->kind == YK_INTEGRATOR_PATH || integrator->kind == YK_INTEGRATOR_WHITTED);
    yk_status rc = li.check(ray_o && ray_d && pixel_xy && sample_index && out_li, sampler, integrator, sample_index, nullptr,
                            accepted ? nullptr : "yk_li implements the Path and Whitted integrators");
    if (rc != YK_OK) return rc;
    const RenderParams& prm = li.prm;  // no CancelRef in it and no clear_cancel before: yk_li neither honours nor reports an interruption
    if (prm.max_depth > YK_CTRL_MAX_DEPTH) return fail(ctx, YK_ERR_INVALID_ARGUMENT, "max_depth too large");
    Staging sg(ctx);
    hipStream_t st = sg.stream;
    if ((rc = li.grow()) != YK_OK) return rc;
    if ((rc = li.raygen(sg, ray_o, ray_d, pixel_xy, sample_index, dimension)) != YK_OK) return rc;
    unsigned long long* counters = ctx->counters.as<unsigned long long>();
    KernelTimer kt;
    kt.ctx = ctx;
    kt.on = false;
    if (prm.integrator == YK_INTEGRATOR_WHITTED)
        launch_whitted(st, trace_grid(ctx), scene->dev, prm, ctx->pixel_xy.as<uint32_t>(), li.d_sample_index, path_buffers(ctx->ws[0], 0), (uint32_t)n,
                       ctx->sample_buf.as<float4>(), ctx->ws[0].spill.as<uint2>(), trace_grid(ctx) * trace_block_size(), error_block(ctx), counters);
    else
        run_bounces(ctx, ctx->ws[0], st, scene, prm, ctx->pixel_xy.as<uint32_t>(), li.d_sample_index, ctx->sample_buf.as<float4>(), kt, counters, false, (uint32_t)n, 0u, false);
    HIP_TRY(ctx, hipGetLastError());
    std::vector<float> tmp(n * 4);
    HIP_TRY(ctx, hipMemcpyAsync(tmp.data(), ctx->sample_buf.p, n * 16, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipMemcpyAsync(li.words, error_block(ctx), sizeof(li.words), hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    if ((rc = li.verdict_and_rgb(tmp, out_li)) != YK_OK) return rc;
    // k_whitted leaves every sample's closest-hit ray count in the sample's fourth word; the wavefront tracks none per sample
    for (size_t i = 0; out_ray_counts && i < n; ++i) {
        out_ray_counts[i] = 0;
        if (prm.integrator == YK_INTEGRATOR_WHITTED) std::memcpy(out_ray_counts + i, tmp.data() + 4 * i + 3, 4);
    }
    return YK_OK;
} YK_CATCH(ctx)

yk_status yk_li_debug(yk_context* ctx, const yk_scene* scene, const yk_sampler_desc* sampler, const yk_integrator_desc* integrator, size_t n,
                      const float* ray_o, const float* ray_d, const uint16_t* pixel_xy, const uint32_t* sample_index, uint32_t dimension, uint32_t ray_cap,
                      float* out_li, uint32_t* out_ray_counts, yk_integrator_ray* out_rays, uint32_t* out_n_rays) try {
    if (!ctx) return YK_ERR_INVALID_ARGUMENT;
    YK_LOCK(ctx);
    LiCall li{ctx, scene, n};
    yk_status rc = li.check(ray_o && ray_d && pixel_xy && sample_index && out_li && out_n_rays && !(ray_cap && !out_rays), sampler, integrator, sample_index,
                            (uint64_t)n * ray_cap > YK_LI_DEBUG_MAX_RECORDS ? "n * ray_cap exceeds YK_LI_DEBUG_MAX_RECORDS" : nullptr,
                            integrator && integrator->kind == YK_INTEGRATOR_PATH ? nullptr : "yk_li_debug implements the Path integrator (the others keep the trait's default)");
    if (rc != YK_OK) return rc;
    (void)hipSetDevice(ctx->device);
    if ((rc = clear_cancel(ctx)) != YK_OK) return rc;
    hipStream_t st = ctx->stream;
    if ((rc = li.grow()) != YK_OK) return rc;
    li.prm.cancel = cancel_ref(ctx);  // an interruption stops the kernels and is reported below
    const size_t n_rec = (size_t)n * ray_cap, rec_bytes = n_rec * sizeof(yk_integrator_ray);
    std::vector<float> tmp(n * 4);
    std::vector<uint32_t> counts(n), n_rays(n);
    Staging sg(ctx);
    yk_integrator_ray* d_rec = sg.temp<yk_integrator_ray>(std::max<size_t>(n_rec, 1));  // copied back only once the sample is known to be whole
    uint32_t* d_counts = sg.output(counts.data(), n);
    uint32_t* d_n_rays = sg.output(n_rays.data(), n);
    if ((rc = li.raygen(sg, ray_o, ray_d, pixel_xy, sample_index, dimension)) != YK_OK) return rc;
    if (rec_bytes) HIP_TRY(ctx, hipMemsetAsync(d_rec, 0, rec_bytes, st));  // the slots a sample leaves unused read as zero
    // path.rs:58-62: min_debug_ray_length, the root box's extent on Bounds3::maximum_extent (bounds.rs:147-156) / 10
    const float* lo = scene->dev.root_bmin;
    const float* hi = scene->dev.root_bmax;
    const float dx = hi[0] - lo[0], dy = hi[1] - lo[1], dz = hi[2] - lo[2];
    const int axis = (dx > dy && dx > dz) ? 0 : (dy > dz ? 1 : 2);
    const float min_len = (hi[axis] - lo[axis]) / 10.0f;
    launch_path_debug(st, trace_grid(ctx), scene->dev, li.prm, ctx->pixel_xy.as<uint32_t>(), li.d_sample_index, path_buffers(ctx->ws[0], 0), (uint32_t)n,
                      ctx->sample_buf.as<float4>(), d_counts, reinterpret_cast<float4*>(d_rec), ray_cap, d_n_rays, min_len,
                      ctx->ws[0].spill.as<uint2>(), trace_grid(ctx) * trace_block_size(), error_block(ctx));
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemcpyAsync(tmp.data(), ctx->sample_buf.p, n * 16, hipMemcpyDeviceToHost, st));
    sg.download();  // counts, n_rays
    HIP_TRY(ctx, hipMemcpyAsync(li.words, error_block(ctx), sizeof(li.words), hipMemcpyDeviceToHost, st));
    if (yk_status fs = sg.finish()) return fs;
    if (ctx->cancel_raised.load(std::memory_order_acquire) || li.words[YK_CTRL_CANCELLED])
        return fail(ctx, YK_ERR_CANCELLED, "interrupted (yk_context_interrupt)");
    if ((rc = li.verdict_and_rgb(tmp, out_li)) != YK_OK) return rc;
    if (rec_bytes) HIP_TRY(ctx, hipMemcpy(out_rays, d_rec, rec_bytes, hipMemcpyDeviceToHost));
    if (out_ray_counts) std::memcpy(out_ray_counts, counts.data(), n * 4);
    std::memcpy(out_n_rays, n_rays.data(), n * 4);
    return YK_OK;
} YK_CATCH(ctx)

}  // extern "C"
