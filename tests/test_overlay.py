"""The overlays of draw_visualizations on the host (no GPU): BoundingVolumeHierarchy::node_bounds, the reference's
world_to_clip and ray line list against independent restatements, and the host instance of the line rule
(yuki_amd/csrc/yk_overlay.h) bit for bit against tests/overlay_ref.py, plus float64 geometry anchors that do not depend
on the rule's float order."""
import ctypes as C

import numpy as np
import pytest

import overlay_ref as ref
from yuki_amd import abi, scenes

M = ref.simple_matrix()


def _one_triangle():
    base = scenes.by_name("city-tiny")
    return scenes.SceneData(points=base.points[:3].copy(), indices=np.array([[0, 1, 2]], dtype=np.uint32), tri_mesh=np.zeros(1, np.uint32),
                            tri_material=np.zeros(1, np.int32), tri_area_light=np.full(1, -1, np.int32), meshes=[(False, False, False)],
                            materials=base.materials[:1], lights=base.lights, camera=base.camera)


def _check_levels(yk, sd):
    sc = yk.Scene(None, sd)
    nodes, _ = sc.export_bvh()
    depth = ref.tree_depth(nodes)
    assert depth == sc.info().tree_depth or depth == sc.info().tree_depth + 1 or depth + 1 == sc.info().tree_depth  # whichever way info counts
    for level in (-1, 0, 1, 2, 5, depth, depth + 3):
        want = ref.node_bounds(nodes, level)
        got = sc.node_bounds(level)
        assert got.shape == want.shape and got.tobytes() == want.tobytes(), (sd.name, level)
    assert len(sc.node_bounds(-1)) == sc.info().n_nodes
    assert len(sc.node_bounds(0)) == 1 and len(sc.node_bounds(depth)) == 0  # the deepest level has only leaves
    sc.close()


def test_node_bounds_root_leaf(yk):
    _check_levels(yk, _one_triangle())
    sc = yk.Scene(None, _one_triangle())
    assert len(sc.node_bounds(-1)) == 1 and len(sc.node_bounds(1)) == 0
    i = sc.info()
    assert sc.node_bounds(0).tobytes() == np.array([list(i.bounds_min), list(i.bounds_max)], np.float32).tobytes()


@pytest.mark.parametrize("name", ["cornell-tris", "city-tiny"])
@pytest.mark.parametrize("method", [abi.SPLIT_SAH, abi.SPLIT_MIDDLE, abi.SPLIT_EQUAL_COUNTS])
@pytest.mark.parametrize("max_shapes", [1, 4])
def test_node_bounds_equals_deque_walk(yk, name, method, max_shapes):
    sd = scenes.by_name(name)
    sd.split_method, sd.max_shapes_in_node = method, max_shapes
    _check_levels(yk, sd)


def test_node_bounds_cap_and_null(yk):
    sc = yk.Scene(None, scenes.by_name("city-tiny"))
    L = yk.lib()
    full = sc.node_bounds(3)
    assert len(full) >= 4
    buf = np.full(6 * 3 + 1, 77.0, np.float32)
    assert L.yk_scene_node_bounds(sc.h, 3, buf.ctypes.data_as(C.c_void_p), 3) == len(full)
    assert buf[:18].tobytes() == full[:3].tobytes() and buf[18] == 77.0
    assert L.yk_scene_node_bounds(None, 3, None, 0) == 0


# --------------------------------------------------------------------------- world_to_clip
@pytest.mark.parametrize("res", [(1920, 1080), (480, 640), (37, 23), (5, 1)])
@pytest.mark.parametrize("axis", [abi.FOV_X, abi.FOV_Y])
def test_world_to_clip_equals_the_reference_statements(yk, oracle, res, axis):
    def tan(x):
        return yk.host_math(2, np.array([x], np.float32))[0]

    assert abs(float(tan(0.5)) - np.tan(0.5)) < 1e-6  # function 2 is tan
    for sd in (scenes.by_name("city-tiny"), scenes.by_name("cornell-tris"), scenes.by_name("cfg2")):
        cam = dict(sd.camera)
        cam["fov_axis"] = axis
        fs = yk.FilmSettings(res=res)
        look_at = np.array(list(oracle.make_camera(cam, res).camera_to_world_inv), np.float32).reshape(4, 4)
        for bounds in (yk.Scene(None, sd).node_bounds(0)[0], np.array([(-1, -2, -3), (4, 5, 6)], np.float32)):
            want = ref.world_to_clip(look_at, cam["position"], axis, cam["fov_degrees"], res, bounds, tan)
            got = yk.overlay_world_to_clip(cam, fs, bounds)
            assert got.tobytes() == want.tobytes(), (sd.name, res, axis)
            # float64 anchors
            m = got.astype(np.float64)
            t = m @ np.array(list(cam["target"]) + [1.0])
            assert abs(t[0] / t[3]) < 1e-5 and abs(t[1] / t[3]) < 1e-5
            b = np.asarray(bounds, np.float64)
            for j in range(8):
                c = m @ np.array([b[(j >> 2) & 1, 0], b[(j >> 1) & 1, 1], b[j & 1, 2], 1.0])
                if c[3] > 0:
                    assert c[2] <= c[3] * (1 + 1e-6)


def test_world_to_clip_argument_checks(yk):
    cam = dict(scenes.by_name("city-tiny").camera)
    fs = yk.FilmSettings(res=(64, 40))
    p = cam["position"]
    for bad in (np.array([p, p], np.float32), np.array([(0, 0, 0), (np.inf, 1, 1)], np.float32), np.array([(np.nan, 0, 0), (1, 1, 1)], np.float32)):
        with pytest.raises(yk.YukiError) as e:
            yk.overlay_world_to_clip(cam, fs, bad)
        assert e.value.status == 1
    out = np.zeros(16, np.float32)
    assert yk.lib().yk_overlay_world_to_clip(None, out.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)) == 1


# --------------------------------------------------------------------------- ray lines
def test_ray_lines_colours_limit_and_infinite_rays(yk):
    rng = np.random.default_rng(3)
    rays = np.zeros(40, abi.INTEGRATOR_RAY_DTYPE)
    rays["o"] = rng.uniform(-3, 3, size=(40, 3))
    rays["d"] = rng.uniform(-1, 1, size=(40, 3))
    rays["t_max"] = rng.uniform(0.1, 9, size=40)
    rays["ray_type"] = np.arange(40) % 5
    rays["t_max"][7] = np.inf
    rays["d"][7] = (0.0, 0.6, 0.8)
    rays["o"][7] = (0.0, 0.0, 1.0)
    got = yk.overlay_ray_lines(rays)
    want = ref.ray_lines(rays)
    assert ref.bits(got["p0"]).tobytes() == ref.bits(want["p0"]).tobytes()
    assert ref.bits(got["p1"]).tobytes() == ref.bits(want["p1"]).tobytes()
    assert got["rgb"].tobytes() == want["rgb"].tobytes()
    for t, rgb in ((yk.RayType.Direct, (1, 1, 1)), (yk.RayType.Reflection, (1, 0, 0)), (yk.RayType.Refraction, (0, 1, 0)), (yk.RayType.Normal, (0, 0, 1)), (yk.RayType.Shadow, (1, 1, 0))):
        assert tuple(got["rgb"][t]) == rgb
    # a miss ray (t_max = inf) becomes a line with a non-finite end, which draws nothing
    assert not np.isfinite(got["p1"][7]).all()
    film = np.zeros((40, 64, 3), np.float32)
    assert not yk.draw_overlay(film, M, lines=got[7:8]).any()
    assert yk.draw_overlay(film, M, lines=got).any()
    # the reference's u16 vertex indices
    big = np.zeros(32769, abi.INTEGRATOR_RAY_DTYPE)
    assert len(yk.overlay_ray_lines(big[:32768])) == 32768
    with pytest.raises(yk.YukiError) as e:
        yk.overlay_ray_lines(big)
    assert e.value.status == 1
    bad = rays[:3].copy()
    bad["ray_type"][1] = 5
    with pytest.raises(yk.YukiError):
        yk.overlay_ray_lines(bad)


# --------------------------------------------------------------------------- the host instance == the restatement
@pytest.mark.parametrize("hw", ref.FILMS)
def test_host_lines_equal_the_restatement(yk, hw):
    h, w = hw
    rng = np.random.default_rng(100 + w)
    film = ref.random_film(rng, h, w)
    drawn = {}
    for name, lines in ref.line_sets(w, h, rng).items():
        got = yk.draw_overlay(film, M, lines=lines)
        want = ref.draw(film, M, lines=lines)
        assert np.array_equal(ref.bits(got), ref.bits(want)), (hw, name)
        rev = lines.copy()
        rev["p0"], rev["p1"] = lines["p1"], lines["p0"]
        assert np.array_equal(ref.bits(yk.draw_overlay(film, M, lines=rev)), ref.bits(got)), (hw, name, "reversed")
        drawn[name] = int((ref.bits(got) != ref.bits(film)).any(axis=2).sum())
        if name in ("empty", "zero length", "outside"):
            assert np.array_equal(ref.bits(got), ref.bits(film)), (hw, name)
    if min(h, w) > 5:
        for name in ("horizontal", "vertical", "diagonal", "centres", "corners", "planes", "behind", "non-finite", "random"):
            assert drawn[name] > 0, (hw, name)  # the set is not vacuous on this film
    print(hw, drawn)


def test_the_order_shows_in_5000_random_lines(yk):
    """Every pixel of 64 x 40 is overdrawn many times: the film depends on the order, and equals the restatement's."""
    rng = np.random.default_rng(164)
    lines = ref.line_sets(64, 40, rng)["random 5000"]
    film = np.zeros((40, 64, 3), np.float32)
    got = yk.draw_overlay(film, M, lines=lines)
    assert np.array_equal(ref.bits(got), ref.bits(ref.draw(film, M, lines=lines)))
    assert ref.bits(got).any(axis=2).all()  # every pixel covered
    assert not np.array_equal(ref.bits(yk.draw_overlay(film, M, lines=lines[::-1].copy())), ref.bits(got))


@pytest.mark.parametrize("hw", ref.FILMS)
def test_host_boxes_equal_the_restatement(yk, hw):
    h, w = hw
    rng = np.random.default_rng(200 + w)
    film = ref.random_film(rng, h, w)
    lines = ref.random_lines(rng, 40)
    for name, boxes in ref.box_sets(rng).items():
        got = yk.draw_overlay(film, M, boxes=boxes)
        assert np.array_equal(ref.bits(got), ref.bits(ref.draw(film, M, boxes=boxes))), (hw, name)
        both = yk.draw_overlay(film, M, lines=lines, boxes=boxes)
        assert np.array_equal(ref.bits(both), ref.bits(ref.draw(film, M, lines=lines, boxes=boxes))), (hw, name, "lines first")
        # lines, then boxes == two calls
        assert np.array_equal(ref.bits(both), ref.bits(yk.draw_overlay(yk.draw_overlay(film, M, lines=lines), M, boxes=boxes)))


def test_box_colours_alternate_and_edges_follow_the_reference(yk):
    boxes = np.array([[(-1, -1, 3), (0, 0, 4)], [(0.2, 0.2, 3), (1, 1, 4)]], np.float32)
    film = yk.draw_overlay(np.zeros((150, 200, 3), np.float32), M, boxes=boxes)
    colours = {tuple(c) for c in film.reshape(-1, 3)}
    assert colours == {(0.0, 0.0, 0.0), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0)}
    only_odd = yk.draw_overlay(np.zeros((150, 200, 3), np.float32), M, boxes=boxes[1:])
    assert {tuple(c) for c in only_odd.reshape(-1, 3)} == {(0.0, 0.0, 0.0), (1.0, 0.0, 0.0)}  # index 0 of its own list


def test_guards_and_untouched_pixels(yk):
    """The film sits between guard floats at a 4-byte offset; untouched pixels keep NaN payloads; nothing outside changes."""
    rng = np.random.default_rng(9)
    h, w = 23, 37
    film = ref.random_film(rng, h, w)
    lines = ref.random_lines(rng, 60)
    boxes = ref.random_boxes(rng, 30)
    buf = np.full(h * w * 3 + 7, 123.25, np.float32)
    buf[3:-4] = film.reshape(-1)
    m = np.ascontiguousarray(M).reshape(16)
    st = yk.lib().yk_overlay_draw(None, m.ctypes.data_as(C.c_void_p), lines.ctypes.data_as(C.c_void_p), len(lines), boxes.ctypes.data_as(C.c_void_p), len(boxes),
                                  C.c_void_p(buf.ctypes.data + 12), w, h)
    assert st == 0
    assert (buf[:3] == 123.25).all() and (buf[-4:] == 123.25).all()
    want = ref.draw(film, M, lines=lines, boxes=boxes)
    assert np.array_equal(ref.bits(buf[3:-4]), ref.bits(want).reshape(-1))
    same = ref.bits(want) == ref.bits(film)
    assert same.all(axis=2).any() and not same.all()


def test_status_codes(yk):
    L = yk.lib()
    vp = C.c_void_p
    film = np.zeros((4, 4, 3), np.float32)
    m = np.ascontiguousarray(M).reshape(16)
    lines = ref.random_lines(np.random.default_rng(1), 2)
    boxes = ref.random_boxes(np.random.default_rng(1), 2)
    pm, pf, pl, pb = m.ctypes.data_as(vp), film.ctypes.data_as(vp), lines.ctypes.data_as(vp), boxes.ctypes.data_as(vp)
    assert L.yk_overlay_draw(None, pm, pl, 2, pb, 2, pf, 4, 4) == 0
    assert L.yk_overlay_draw(None, pm, None, 0, None, 0, pf, 4, 4) == 0
    assert L.yk_overlay_draw(None, pm, pl, 2, pb, 2, None, 4, 4) == 1  # NULL film
    assert L.yk_overlay_draw(None, pm, pl, 2, pb, 2, pf, 0, 4) == 1  # zero resolution
    assert L.yk_overlay_draw(None, pm, pl, 2, pb, 2, pf, 4, 0) == 1
    assert L.yk_overlay_draw(None, pm, None, 2, pb, 2, pf, 4, 4) == 1  # NULL list with a count
    assert L.yk_overlay_draw(None, pm, pl, 2, None, 2, pf, 4, 4) == 1
    assert L.yk_overlay_draw(None, None, pl, 2, pb, 2, pf, 4, 4) == 1
    assert L.yk_overlay_draw_device(None, pm, pl, 2, pb, 2, pf, 4, 4, None) == 1  # no context
    assert L.yk_sizeof(16) == 36 == abi.OVERLAY_LINE_DTYPE.itemsize


# --------------------------------------------------------------------------- geometry anchors (float64)
EPS = 2.0 ** -6  # px: window coordinates < 2^12, fewer than 16 roundings of at most 2^-12 px each = 2^-8, times 4 of room


def _anchor_lines(rng, n):
    """Ends with |coordinates| <= 16, w >= 1, strictly inside the view volume of simple_matrix()."""
    z = rng.uniform(1.0, 16.0, size=(2, n))
    xy = rng.uniform(-0.999, 0.999, size=(2, n, 2)) * z[:, :, None]
    p = np.concatenate([xy, z[:, :, None]], axis=2).astype(np.float32)
    return ref.make_lines(p[0], p[1], rgb=np.ones((n, 3)))


@pytest.mark.parametrize("res", [(4096, 4096), (1920, 1080), (37, 23), (3, 4096)])
def test_geometry_anchors(yk, res):
    """One line alone in a zero film: every drawn pixel lies within half a pixel (+ EPS) of the exact line, every major-axis
    pixel centre strictly inside the exact extent (by EPS) has exactly one pixel, and none lies beyond the extent.  The
    lines are random (none within 1 px of a diagonal, where the major axis itself is a rounding decision), plus axis-aligned
    and steep ones."""
    rx, ry = res
    rng = np.random.default_rng(rx * 7 + ry)
    lines = _anchor_lines(rng, 24)
    lines["p1"][0, 1] = lines["p0"][0, 1] * lines["p1"][0, 2] / lines["p0"][0, 2]  # (nearly) horizontal in the window
    lines["p1"][1, 0] = lines["p0"][1, 0] * lines["p1"][1, 2] / lines["p0"][1, 2]  # (nearly) vertical
    m64 = M.astype(np.float64)
    m32 = np.ascontiguousarray(M).reshape(16)
    film = np.zeros((ry, rx, 3), np.float32)
    checked = 0
    for i in range(len(lines)):
        ends = []
        for p in (lines["p0"][i], lines["p1"][i]):
            c = m64 @ np.append(p.astype(np.float64), 1.0)
            assert c[3] >= 1.0 and (np.abs(c[:3]) < c[3]).all()
            ends.append((((c[0] / c[3]) * 0.5 + 0.5) * rx, ((c[1] / c[3]) * 0.5 + 0.5) * ry))
        (x0, y0), (x1, y1) = ends
        if abs(abs(x1 - x0) - abs(y1 - y0)) < 1.0:
            continue
        x_major = abs(x1 - x0) >= abs(y1 - y0)
        a, b, m_a, m_b = (x0, x1, y0, y1) if x_major else (y0, y1, x0, x1)
        if a > b:
            a, b, m_a, m_b = b, a, m_b, m_a
        one = lines[i : i + 1].copy()
        assert yk.lib().yk_overlay_draw(None, m32.ctypes.data_as(C.c_void_p), one.ctypes.data_as(C.c_void_p), 1, None, 0, film.ctypes.data_as(C.c_void_p), rx, ry) == 0
        bx0, by0 = max(int(min(x0, x1)) - 2, 0), max(int(min(y0, y1)) - 2, 0)  # look where the line can be; the rest is checked once at the end
        ys, xs = np.nonzero(film[by0 : int(max(y0, y1)) + 3, bx0 : int(max(x0, x1)) + 3, 0])
        ys, xs = ys + by0, xs + bx0
        film[ys, xs] = 0.0  # one film for all the lines: each is drawn alone
        k, r = (xs, ys) if x_major else (ys, xs)
        exact = m_a + (k + 0.5 - a) * (m_b - m_a) / (b - a)
        assert (np.abs(r + 0.5 - exact) <= 0.5 + EPS).all(), (res, i)
        assert ((k + 0.5 >= a - EPS) & (k + 0.5 < b + EPS)).all(), (res, i)
        counts = np.bincount(k, minlength=(rx if x_major else ry))
        inside = np.arange(len(counts))
        inside = inside[(inside + 0.5 >= a + EPS) & (inside + 0.5 < b - EPS)]
        assert (counts[inside] == 1).all(), (res, i)
        assert (counts <= 1).all() or (counts[inside] == 1).all()
        checked += 1
    assert checked >= 16
    assert not film.any()  # no line drew outside the box searched for it
