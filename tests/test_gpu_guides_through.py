"""Guides through glass on the MI355X (yk_render_guides_through, yuki_amd/csrc/yk_guides_through.h): max_through = 0 is
render_guides_ids byte for byte; guides, ids and `through` equal the independent restatement (tests/guides_through_ref.py:
oracle surfaces and lobes, numpy float32 spawn rule and T) bit for bit on every scene, bound and context; the second
segment ties to the device's own yk_surface + yk_bsdf_sample; batches and repeated calls change no byte; the device form
writes between guard words, takes each output as NULL, refuses what the header says and is ordered on a caller's stream;
and the records go through surface_albedo_device and denoise_device(albedo=) with the host instances' bytes."""
import ctypes as C

import numpy as np
import pytest

import guides_through_ref as ref
from test_gpu_temporal import GUARD, _between_guards, _payload
from yuki_amd import abi, scenes

pytestmark = pytest.mark.gpu
F = np.float32
SF = abi.SURFACE_FIELDS

SCENES = {"cornell": (48, 48), "glass-balls": (48, 48), "city-small": (96, 54)}
SCENES.update({"glass-" + v: ref.RES for v in ref.VARIANTS})
BOUNDS = (1, 2, 4, 8)


def _scene_data(name):
    variant = name[len("glass-") :] if name.startswith("glass-") else None
    return ref.slab_scene(variant) if variant in ref.VARIANTS else scenes.by_name(name)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@pytest.fixture(scope="module")
def contexts(yk):
    """The two closest-hit routes of the stage calls ("trace_stage_kernel" 0 and 1: the tie test's yk_surface goes through
    them) and the small-batch context: 256 paths a batch, so the 851 rays of a 37 x 23 film are four batches."""
    c = {0: yk.Context(0, trace_stage_kernel=0), 1: yk.Context(0, trace_stage_kernel=1), "small": yk.Context(0, sample_buf_cap=1 << 20, batch_paths=256, streams=2)}
    yield c
    for v in c.values():
        v.close()


@pytest.fixture(scope="module")
def views(yk, oracle, contexts):
    """name -> dict(sd, sc, cam, fs, want): the device scene (it belongs to the device: every context renders it) and the
    restatement's (guides, ids, through, branch) for every bound, computed once and left unchanged."""
    out = {}
    for name, res in SCENES.items():
        sd = _scene_data(name)
        fs = yk.FilmSettings(res=res, tile_dim=16)
        cam = yk.Camera(sd.camera, fs)
        osc = oracle.OracleScene(sd)
        want = {}
        for mt in (0,) + BOUNDS:
            want[mt] = ref.guides_through(oracle, osc, sd, cam, res, mt)
            for a in want[mt]:
                a.setflags(write=False)
        osc.close()
        out[name] = dict(sd=sd, sc=yk.Scene(contexts[0], sd), cam=cam, fs=fs, want=want)
    yield out
    for v in out.values():
        v["sc"].close()


def _assert_records(got, want, what):
    g, i, t = got
    wg, wi, wt = want[:3]
    assert np.array_equal(t, wt), (what, "through", int((t != wt).sum()))
    for k in ("ns", "hit", "p", "t"):
        bad = _bits(g[k]) != _bits(wg[k])
        assert not bad.any(), (what, k, int(bad.sum()), np.argwhere(bad)[:3])
    assert np.array_equal(i["shape"], wi["shape"]), (what, "shape")
    assert np.array_equal(_bits(i["b"]), _bits(wi["b"])), (what, "b")


@pytest.mark.parametrize("name,res", [("cornell", (48, 48)), ("city-tiny", (100, 60))])
def test_zero_is_render_guides_ids(yk, contexts, name, res):
    sd = scenes.by_name(name)
    fs = yk.FilmSettings(res=res, tile_dim=16)
    cam = yk.Camera(sd.camera, fs)
    sc = yk.Scene(contexts[0], sd)
    guides, ids = yk.render_guides_ids(contexts[0], sc, cam, fs)
    for c in contexts.values():
        g, i, t = yk.render_guides_through(c, sc, cam, fs, max_through=0)
        assert g.tobytes() == guides.tobytes() and i.tobytes() == ids.tobytes() and not t.any()
    assert guides["hit"].any()
    sc.close()


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("name", list(SCENES))
def test_parity_with_the_restatement(yk, contexts, views, name, mode):
    v = views[name]
    assert same(yk.render_guides_through(contexts[mode], v["sc"], v["cam"], v["fs"], 0)[0], v["want"][0][0])
    for mt in BOUNDS:
        got = yk.render_guides_through(contexts[mode], v["sc"], v["cam"], v["fs"], mt)
        _assert_records(got, v["want"][mt], (name, mode, mt))
    assert (v["want"][8][2] >= 1).any() or name == "glass-black"


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("name", ["glass-slab", "glass-prism", "glass-mirror", "glass-balls"])
def test_second_segment_ties_to_the_stage_calls(yk, contexts, views, name, mode):
    """Device only: for the pixels that crossed an interface, max_through = 1's record is yk_surface of the ray built from
    yk_surface of the camera ray and yk_bsdf_sample's direction (u0 = 0.75, or 0.25 where the restatement reflected)."""
    ctx, v = contexts[mode], views[name]
    sd, sc, cam, fs = v["sd"], v["sc"], v["cam"], v["fs"]
    w, h = fs.res
    g, i, t = (a.reshape(-1) for a in yk.render_guides_through(ctx, sc, cam, fs, 1))
    branch0 = v["want"][1][3].reshape(-1, ref.MAX + 1)[:, 0]
    px = np.flatnonzero(t == 1)
    assert len(px) > 20
    o, d = yk.camera_rays(ctx, cam, yk.SamplerType.Stratified((1, 1), False), (0, 0, w, h), 0)
    rec0 = yk.surface(ctx, sc, o[px], d[px], 0)
    assert (rec0[:, SF["hit"]] == 1).all()
    wi = np.zeros((len(px), 3), F)
    for m in np.unique(rec0[:, SF["material"]]).astype(int):
        rows = np.flatnonzero(rec0[:, SF["material"]] == m)
        u = np.zeros((len(rows), 2), F)
        u[:, 0] = np.where(branch0[px[rows]] == ref.TRANSMIT, 0.75, 0.25)
        s = yk.bsdf_sample(ctx, ref._material_desc(sd.materials[m]), rec0[rows, SF["n"]], rec0[rows, SF["ns"]], rec0[rows, SF["dpdus"]], -d[px[rows]], u)
        assert (s[:, 6] != 0).all()
        wi[rows] = s[:, 0:3]
    o1 = np.stack([ref.spawn_origin(rec0[k, SF["p"]], rec0[k, SF["n"]], wi[k]) for k in range(len(px))])
    rec1 = yk.surface(ctx, sc, o1, wi, 0)
    hit = rec1[:, SF["hit"]] != 0
    assert hit.any()
    assert np.array_equal(g["hit"][px] != 0, hit)
    assert np.array_equal(_bits(g["ns"][px][hit]), _bits(rec1[hit, SF["ns"]])) and np.array_equal(_bits(g["p"][px][hit]), _bits(rec1[hit, SF["p"]]))
    T = (rec0[:, SF["t"]] + rec1[:, SF["t"]]).astype(F)
    assert np.array_equal(_bits(g["t"][px][hit]), _bits(T[hit]))
    assert np.array_equal(i["shape"][px][hit], rec1[hit, SF["shape"]].astype(np.uint32)) and (i["shape"][px][~hit] == abi.SURFACE_NONE).all()
    assert np.array_equal(_bits(i["b"][px][hit]), _bits(rec1[hit, SF["b"]]))
    assert not _bits(g[px][~hit].view(F)).any()


@pytest.mark.parametrize("name", ["glass-two", "glass-prism", "city-small"])
def test_batches_and_repeats_change_no_byte(yk, contexts, views, name):
    v = views[name]
    w, h = v["fs"].res
    assert name == "city-small" or ((w * h) % 64 and (w * h) % 256)
    for mt in (2, 8):
        a = yk.render_guides_through(contexts[0], v["sc"], v["cam"], v["fs"], mt)
        b = yk.render_guides_through(contexts[0], v["sc"], v["cam"], v["fs"], mt)
        s = yk.render_guides_through(contexts["small"], v["sc"], v["cam"], v["fs"], mt)
        for x, y, z in zip(a, b, s):
            assert x.tobytes() == y.tobytes() == z.tobytes(), (name, mt)


def test_device_form_guards_nulls_refusals_and_stream_order(yk, contexts, views):
    import torch

    ctx, v = contexts[0], views["glass-two"]
    sc, cam, fs = v["sc"], v["cam"], v["fs"]
    w, h = fs.res
    n = w * h
    want = [a.view(np.uint32).reshape(-1) for a in yk.render_guides_through(ctx, sc, cam, fs, 4)]
    s = torch.cuda.Stream()
    d_g, d_i, d_t = _between_guards(torch, 8 * n, 4), _between_guards(torch, 4 * n, 8), _between_guards(torch, n, 3)
    G, I, T = d_g.data_ptr() + 16, d_i.data_ptr() + 32, d_t.data_ptr() + 12
    torch.cuda.synchronize()
    ctx.render_guides_through_device(sc, cam, fs.res, G, I, T, max_through=4, stream=s.cuda_stream)
    s.synchronize()
    assert np.array_equal(_payload(d_g, 4, 8 * n), want[0]) and np.array_equal(_payload(d_i, 8, 4 * n), want[1]) and np.array_equal(_payload(d_t, 3, n), want[2])
    # each output NULL in turn
    for drop in range(3):
        bufs = [_between_guards(torch, 8 * n, 4), _between_guards(torch, 4 * n, 4), _between_guards(torch, n, 1)]
        ptrs = [bufs[0].data_ptr() + 16, bufs[1].data_ptr() + 16, bufs[2].data_ptr() + 4]
        ptrs[drop] = None
        torch.cuda.synchronize()
        ctx.render_guides_through_device(sc, cam, fs.res, *ptrs, max_through=4, stream=s.cuda_stream)
        s.synchronize()
        for k, (lead, words) in enumerate([(4, 8 * n), (4, 4 * n), (1, n)]):
            got = _payload(bufs[k], lead, words)
            assert (got == np.uint32(GUARD)).all() if k == drop else np.array_equal(got, want[k]), (drop, k)
    # refusals: nothing is launched, the buffers keep their bytes
    bad = [(None, None, None, 4), (G, I, T, 9), (G + 4, I, T, 4), (G, I + 8, T, 4), (G, I, T + 2, 4), (G, G + 16, T, 4), (G, I, G + 32, 4), (G, I, I + 4 * n, 4), (I + 16 * n - 16, I, T, 4)]
    for g_ptr, i_ptr, t_ptr, mt in bad:
        with pytest.raises(yk.YukiError) as e:
            ctx.render_guides_through_device(sc, cam, fs.res, g_ptr, i_ptr, t_ptr, max_through=mt)
        assert e.value.status == 1, (g_ptr, i_ptr, t_ptr, mt)
    L = yk.lib()
    assert L.yk_render_guides_through(ctx.h, sc.h, C.byref(cam.matrices), w, h, 4, None, None, None) == 1
    assert L.yk_render_guides_through(ctx.h, sc.h, C.byref(cam.matrices), w, h, 9, None, None, want[2].ctypes.data) == 1
    torch.cuda.synchronize()
    assert np.array_equal(_payload(d_g, 4, 8 * n), want[0]) and np.array_equal(_payload(d_i, 8, 4 * n), want[1]) and np.array_equal(_payload(d_t, 3, n), want[2])
    # ordering on the caller's stream: a fill before the call and a copy after it, no host wait in between
    with torch.cuda.stream(s):
        d_g.fill_(GUARD)
        d_t.fill_(GUARD)
        ctx.render_guides_through_device(sc, cam, fs.res, G, None, T, max_through=4, stream=s.cuda_stream)
        g_copy, t_copy = d_g.clone(), d_t.clone()
    s.synchronize()
    assert np.array_equal(_payload(g_copy, 4, 8 * n), want[0]) and np.array_equal(_payload(t_copy, 3, n), want[2])


def test_write_output_renders_the_guides_itself(yk, contexts, views, tmp_path):
    """guides_through=(scene, camera[, max_through]) on write_output / write_preview is guides= (and albedo=) of the same call."""
    ctx, v = contexts[0], views["glass-slab"]
    sc, cam, fs = v["sc"], v["cam"], v["fs"]
    w, h = fs.res
    film = np.random.default_rng(12).random((h, w, 3), dtype=np.float32)
    p = yk.DenoiseParams(iterations=2, sigma_plane=0.06)
    guides, ids, _ = yk.render_guides_through(ctx, sc, cam, fs, 2)
    albedo = yk.surface_albedo(sc, ids, ctx)
    a, b, c, d = (tmp_path / n for n in ("a.exr", "b.exr", "c.exr", "d.exr"))
    yk.write_output(a, film, yk.ToneMapType.Raw, settings=fs, ctx=ctx, denoise=p, guides=guides)
    yk.write_output(b, film, yk.ToneMapType.Raw, settings=fs, ctx=ctx, denoise=p, guides_through=(sc, cam, 2))
    yk.write_output(c, film, yk.ToneMapType.Raw, settings=fs, ctx=ctx, denoise=p, guides=guides, albedo=albedo)
    yk.write_output(d, film, yk.ToneMapType.Raw, settings=fs, ctx=ctx, denoise=p, guides_through=(sc, cam, 2), albedo=True)
    assert a.read_bytes() == b.read_bytes() != c.read_bytes() and c.read_bytes() == d.read_bytes()
    yk.write_preview(tmp_path / "a.png", film, settings=fs, ctx=ctx, denoise=p, guides=yk.render_guides_through(ctx, sc, cam, fs)[0])
    yk.write_preview(tmp_path / "b.png", film, settings=fs, ctx=ctx, denoise=p, guides_through=(sc, cam))  # the default bound, 4
    assert (tmp_path / "a.png").read_bytes() == (tmp_path / "b.png").read_bytes()
    with pytest.raises(ValueError):
        yk.write_output(a, film, settings=fs, ctx=ctx, denoise=p, guides=guides, guides_through=(sc, cam))


def test_the_chain_takes_the_records(yk, contexts, views):
    """Through-guides and ids into surface_albedo_device and denoise_device(albedo=): the host instances' bytes on the same
    records, and an albedo that is no longer all ones behind the pane."""
    import torch

    ctx, v = contexts[0], views["glass-slab"]
    sc, cam, fs = v["sc"], v["cam"], v["fs"]
    w, h = fs.res
    n = w * h
    guides, ids, through = yk.render_guides_through(ctx, sc, cam, fs, 4)
    film = np.random.default_rng(11).random((h, w, 3), dtype=np.float32)
    p = yk.DenoiseParams(iterations=3, sigma_plane=0.06)
    want_albedo = yk.surface_albedo(sc, ids)
    want = yk.denoise(film, guides, p, 16, None, None, want_albedo)
    first_albedo = yk.surface_albedo(sc, yk.render_guides_ids(ctx, sc, cam, fs)[1])
    behind = through >= 1
    assert behind.sum() > 100 and (first_albedo["known"][behind] == 0).all() and (want_albedo["known"][behind] == 1).mean() > 0.9
    s = torch.cuda.Stream()
    d_g, d_i = _between_guards(torch, 8 * n, 4), _between_guards(torch, 4 * n, 4)
    d_a, d_film, d_out = _between_guards(torch, 4 * n, 4), _between_guards(torch, 3 * n, 4, film), _between_guards(torch, 3 * n, 4)
    torch.cuda.synchronize()
    ctx.render_guides_through_device(sc, cam, fs.res, d_g.data_ptr() + 16, d_i.data_ptr() + 16, None, max_through=4, stream=s.cuda_stream)
    ctx.surface_albedo_device(sc, d_i.data_ptr() + 16, fs.res, d_a.data_ptr() + 16, stream=s.cuda_stream)
    ctx.denoise_device(d_film.data_ptr() + 16, d_g.data_ptr() + 16, fs.res, p, 16, None, d_out.data_ptr() + 16, stream=s.cuda_stream, albedo=d_a.data_ptr() + 16)
    s.synchronize()
    assert np.array_equal(_payload(d_a, 4, 4 * n), want_albedo.view(np.uint32).reshape(-1))
    assert np.array_equal(_payload(d_out, 4, 3 * n), want.view(np.uint32).reshape(-1))
