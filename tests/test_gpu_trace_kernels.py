"""Every traversal kernel on the device, through the stage entry points' "trace_stage_kernel" option
(yk_stages.cpp): the generic kernels in their API flavour (0) and in the render loop's (1), each on binary and
4-wide nodes, and the wave-packet kernels (2).  Each against the oracle bit for bit (shape ids everywhere, t
in mode 0, any-hit verdicts) and, on the rays where the answer is robust, against the float64 brute force of
tests/trace_ref.py.  Mode 2 additionally with rays ordered so that every 64-ray packet has a given make-up."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import test_trace_reference as tr
import trace_ref
from yuki_amd import scenes

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))

pytestmark = pytest.mark.gpu

F = np.float32
CONFIGS = [(0, 0), (0, 1), (1, 0), (1, 1), (2, None)]  # (trace_stage_kernel, wide_bvh)
YK_ERR_INVALID_ARGUMENT = 1


def _bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


@pytest.fixture(scope="module")
def contexts(yk):
    made = {}

    def get(mode, wide):
        if (mode, wide) not in made:
            made[(mode, wide)] = yk.Context(0, trace_stage_kernel=mode, **({} if wide is None else {"wide_bvh": wide}))
        return made[(mode, wide)]

    yield get
    for c in made.values():
        c.close()


def closest_ids(yk, sc, o, d, t_max=None, want_t=False):
    """yk_trace_closest with shape ids (and t if asked): Scene.intersect always asks for t and barycentrics."""
    o = np.ascontiguousarray(o, dtype=F)
    d = np.ascontiguousarray(d, dtype=F)
    n = o.shape[0]
    shape = np.zeros(n, dtype=np.int32)
    t = np.zeros(n, dtype=F) if want_t else None
    tm = None if t_max is None else np.ascontiguousarray(t_max, dtype=F)
    p = lambda a: None if a is None else C.c_void_p(a.ctypes.data)  # noqa: E731
    yk.check(yk.lib().yk_trace_closest(sc.ctx.h, sc.h, n, p(o), p(d), p(tm), p(shape), p(t), None, None, None, None), sc.ctx.h)
    return shape, t


def run_closest(yk, mode, sc, osc, ref, label, o, d, t_max=None):
    """Device against the oracle (ids; t bits in mode 0), then against the f64 reference on robust rays."""
    shape, t = closest_ids(yk, sc, o, d, t_max, want_t=mode == 0)
    w = osc.intersect(o, d, t_max)
    bad = shape != w["shape"]
    assert not bad.any(), (label, mode, int(bad.sum()), np.nonzero(bad)[0][:5], shape[bad][:5], w["shape"][bad][:5])
    if mode == 0:
        hit = w["shape"] >= 0
        assert np.array_equal(_bits(t[hit]), _bits(w["t"][hit])), (label, "t bits")
    if ref is not None:
        tr.check_closest(ref, label, o, d, t_max, shape, t)


def run_any(mode, sc, osc, ref, label, o, d, t_max, al):
    got = sc.any_intersect(o, d, t_max, al)
    want = osc.any_intersect(o, d, t_max, al)
    bad = got != want
    assert not bad.any(), (label, mode, int(bad.sum()), np.nonzero(bad)[0][:5])
    if ref is not None:
        tr.check_any(ref, label, o, d, t_max, al, got)


# ------------------------------------------------------------------ every configuration, the shared ray sets
@pytest.mark.parametrize("mode,wide", CONFIGS)
@pytest.mark.parametrize("name", ["cornell", "glass-balls", "glass-balls-xf", "city-small", "cfg2", "deep-chain-60", "coplanar-slabs", "single-triangle", "duplicated-triangles", "fuzz-1", "fuzz-2", "fuzz-3"])
def test_trace_kernel_matches_oracle_and_f64(yk, oracle, contexts, name, mode, wide):
    sd = tr.scene_by_name(name)
    sc = yk.Scene(contexts(mode, wide), sd)
    osc = oracle.OracleScene(sd)
    # ties between coplanar surfaces make the slabs scene's shape ambiguous: oracle only (its t: test_trace_reference.py)
    ref = None if name == "coplanar-slabs" else trace_ref.TraceRef(sd)
    closest, anyhit = tr.ray_sets(oracle, sd, name, scale=0.5 if name == "cfg2" else 1.0)
    for label, o, d, tm in closest:
        if tm is not None and mode != 0:
            continue  # refused (test_mode_refusals)
        run_closest(yk, mode, sc, osc, ref, label, o, d, tm)
    for label, o, d, tm, al in anyhit:
        run_any(mode, sc, osc, ref, label, o, d, tm, al)
    sc.close()


@pytest.mark.parametrize("kernel", [1, 2])
@pytest.mark.parametrize("seed", [0, 1, 5, 12, 33, 34])
def test_stage_fuzz_through_kernel(oracle, seed, kernel):
    """tools/stage_fuzz.py's degenerate rays (zero direction components, origins on box faces and vertices,
    rays along edges, t_max at exact hit distances for the any-hit kernels) through modes 1 and 2."""
    import stage_fuzz

    assert stage_fuzz.check_seed(oracle, seed, kernel) == []


# ------------------------------------------------------------------ packet make-up (mode 2)
def _sign_zero_pairs(sd, n, seed):
    """Packets of two interleaved groups whose directions differ only by +0.0 / -0.0 in one component:
    1/d is +inf against -inf there, so the lanes fall in different direction-sign groups."""
    rng = np.random.default_rng(seed)
    lo, hi = sd.points.min(axis=0), sd.points.max(axis=0)
    o = (lo + rng.uniform(0, 1, (n, 3)) * (hi - lo)).astype(F)
    d = rng.normal(size=(n, 3)).astype(F)
    ax = rng.integers(0, 3, n // 64).repeat(64)
    d[np.arange(n), ax] = np.where(np.arange(n) % 2 == 0, F(0.0), F(-0.0))
    return o, d


def _root_misses_between_hits(sd, n, seed):
    """Lanes that miss the root box (outside it, looking away) interleaved with lanes aimed at centroids."""
    rng = np.random.default_rng(seed)
    lo, hi = sd.points.min(axis=0).astype(np.float64), sd.points.max(axis=0).astype(np.float64)
    ho, hd = tr.centroid_rays(sd, n, seed)
    c = (lo + hi) / 2
    u = rng.normal(size=(n, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    mo = (c + u * (np.linalg.norm(hi - lo) + 1.0)).astype(F)
    md = (u * rng.uniform(0.5, 2.0, (n, 1))).astype(F)
    odd = np.arange(n) % 2 == 1
    return np.where(odd[:, None], mo, ho), np.where(odd[:, None], md, hd)


def packet_sets(oracle, sd, name):
    """-> [(label, o, d)], each set ordered so that the 64-ray packets have the make-up the label names."""
    import stage_fuzz

    out = []
    if sd.camera is not None:
        res = (16, 12)
        pix = np.random.default_rng(1).permutation(res[0] * res[1])[:24]
        out.append(("one pixel's camera bundle per packet", *tr.pixel_bundles(oracle, sd, res, pix)))
    out.append(("64 random rays per packet", *tr.random_rays(sd, 64 * 32, 2)))
    out.append(("+0.0 / -0.0 groups", *_sign_zero_pairs(sd, 64 * 32, 3)))
    out.append(("root-box misses between hits", *_root_misses_between_hits(sd, 64 * 32, 4)))
    out.append(("stage_fuzz degenerate rays", *stage_fuzz.rays_for(sd, np.random.default_rng(5), n=64 * 24)))
    for n in (1, 63, 64, 65, 4097):
        out.append((f"partial last packet, batch of {n}", *tr.random_rays(sd, n, 6 + n)))
    return out


@pytest.mark.parametrize("name", ["cornell", "glass-balls-xf", "city-small", "coplanar-slabs"])
def test_packet_kernels_by_packet_makeup(yk, oracle, contexts, name):
    sd = tr.scene_by_name(name)
    sc = yk.Scene(contexts(2, None), sd)
    osc = oracle.OracleScene(sd)
    ref = None if name == "coplanar-slabs" else trace_ref.TraceRef(sd)
    sets = packet_sets(oracle, sd, name)
    if name == "coplanar-slabs":
        # not camera rays, every sign group: the relaxed deferred bound (yk_geom.h) on rays whose tie hits raise t_max
        sets.append(("coplanar rays, all sign groups", *tr.coplanar_rays(64 * 64, 7)))
    rng = np.random.default_rng(8)
    for label, o, d in sets:
        run_closest(yk, 2, sc, osc, ref, label, o, d)
        tm = rng.uniform(0.0, 3.0, len(o)).astype(F)
        al = np.where(rng.random(len(o)) < 0.5, rng.integers(-1, max(1, len(sd.lights)), len(o)), -1).astype(np.int32)
        run_any(2, sc, osc, ref, label + " (any)", o, d, tm, al)
    seg = tr.shadow_segments(sd, 64 * 16, 9)
    if seg is not None:
        so, sdir, stm, right, wrong = seg
        al = np.where(np.arange(len(so)) % 3 == 0, wrong, right).astype(np.int32)
        run_any(2, sc, osc, ref, "shadow segments, area_light on some lanes", so, sdir, stm, al)
    sc.close()


# ------------------------------------------------------------------ the packet stack's boundary
def test_packet_stack_at_depth_64(yk, oracle, contexts):
    """deep-chain-64: a +x ray defers 63 children before its first leaf, so every wave of a block holds 63
    entries of its 64-entry LDS stack at once; at least four full waves of such rays per block of the grid."""
    import torch

    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    sd = scenes.by_name("deep-chain-64")
    sc = yk.Scene(contexts(2, None), sd)
    assert sc.info().tree_depth == 64
    n = n_cu * 8 * 256  # packet_blocks_per_cu() = 8 blocks of 256 lanes per CU
    rng = np.random.default_rng(10)
    o = np.stack([np.full(n, -1.0), rng.uniform(-0.5, 0.5, n), rng.uniform(-1.5, 0.5, n)], axis=1).astype(F)  # inside every triangle
    d = np.zeros((n, 3), dtype=F)
    d[:, 0] = 1.0
    d[n // 2 :, 1:] = rng.uniform(0.0, 1e-3, (n - n // 2, 2))  # still one sign group
    shape, _ = closest_ids(yk, sc, o, d)
    want = oracle.OracleScene(sd).intersect(o, d)["shape"]
    assert np.array_equal(shape, want)
    assert (want >= 0).all()  # every ray crosses all 64 triangles (x = 3^-k: most of them tie at t = 1 in f32)
    ref = trace_ref.TraceRef(sd)
    sel = rng.permutation(n)[:4000]
    tr.check_closest(ref, "deep-chain-64", o[sel], d[sel], None, shape[sel], None)
    tm = np.full(n, 2.0, dtype=F)
    assert np.array_equal(sc.any_intersect(o, d, tm), oracle.OracleScene(sd).any_intersect(o, d, tm))
    sc.close()


def test_mode_refusals(yk, contexts):
    """A mode refuses what it cannot honour; it never falls back to another kernel."""
    sd = scenes.by_name("cornell")
    o, d = tr.random_rays(sd, 256, 11)
    tm = np.ones(256, dtype=F)
    for mode in (1, 2):
        sc = yk.Scene(contexts(mode, None), sd)
        with pytest.raises(yk.YukiError) as e:
            sc.intersect(o, d)  # asks for t and barycentrics
        assert e.value.status == YK_ERR_INVALID_ARGUMENT
        with pytest.raises(yk.YukiError) as e:
            sc.intersect(o, d, counters=True)
        assert e.value.status == YK_ERR_INVALID_ARGUMENT
        with pytest.raises(yk.YukiError) as e:
            closest_ids(yk, sc, o, d, t_max=tm)
        assert e.value.status == YK_ERR_INVALID_ARGUMENT
        closest_ids(yk, sc, o, d)  # ids only: accepted
        sc.close()
    deep = yk.Scene(contexts(2, None), scenes.by_name("deep-chain-65"))
    assert deep.info().tree_depth == 65
    o = np.tile(np.array([[-1.0, 0.1, 0.2]], dtype=F), (64, 1))
    d = np.tile(np.array([[1.0, 0.0, 0.0]], dtype=F), (64, 1))
    with pytest.raises(yk.YukiError) as e:
        closest_ids(yk, deep, o, d)
    assert e.value.status == YK_ERR_INVALID_ARGUMENT
    with pytest.raises(yk.YukiError) as e:
        deep.any_intersect(o, d, np.full(64, 2.0, dtype=F))
    assert e.value.status == YK_ERR_INVALID_ARGUMENT
    deep.close()
    c = contexts(0, None)
    for bad in (-1, 3):
        with pytest.raises(yk.YukiError):
            c.set_option("trace_stage_kernel", bad)
