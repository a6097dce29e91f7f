"""yk_load_mitsuba / yk_load_scene (scene/mitsuba/*.rs, app/util.rs:15-63) against the independent restatement in
tests/mitsuba_ref.py, bit for bit, on files written at test time (tests/mitsuba_files.py).

Parity unpinned: the reference holds no tests or sample files for this loader; what these tests pin is that two
independent implementations of its source text agree exactly, that float64 anchors computed from the files' numbers
agree with both, and the behaviours the reference spells out (quirks included)."""
import os
import re
import time
import xml.etree.ElementTree as ET

import numpy as np
import pytest

from yuki_amd import abi, loaders
from yuki_amd._ffi import YukiError

import mitsuba_files as mf
import scene_files as sf

ERR_INVALID_ARGUMENT, ERR_UNSUPPORTED = 1, 5  # yk_status, include/yuki_hip.h


@pytest.fixture(scope="module")
def mr(oracle):
    import mitsuba_ref

    return mitsuba_ref


# ----------------------------------------------------------------------------- field for field
def _xf64(node):
    """A <transform> element in float64: every child pre-multiplies (transform.rs)."""
    T = np.eye(4)
    for c in node:
        M = np.eye(4)
        if c.tag == "rotate":
            a = np.array([float(c.get(k, "0")) for k in "xyz"])
            a /= np.linalg.norm(a)
            th = np.deg2rad(float(c.get("angle")))
            K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
            M[:3, :3] = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)
        elif c.tag == "translate":
            M[:3, 3] = [float(v) for v in c.get("value").split(" ")]
        elif c.tag == "scale":
            v = [float(x) for x in c.get("value").split(" ")]
            M[:3, :3] = np.diag(v * 3 if len(v) == 1 else v)
        elif c.tag == "matrix":
            M = np.array([float(x) for x in c.get("value").split(" ")]).reshape(4, 4)
        T = M @ T
    return T


MIRROR = np.diag([-1.0, 1.0, 1.0, 1.0])
REL = 2e-5  # fifty-odd f32 operations at 2^-24 each stay below 3e-6, the libm calls below one ulp more


def _close(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return np.linalg.norm(got - want) <= REL * np.linalg.norm(want)


@pytest.mark.parametrize("fov_axis", ["x", "y"])
def test_hand_written_scene_field_for_field(tmp_path, mr, fov_axis):
    from oracle import loaders as ol

    p = mf.write_hand_scene(str(tmp_path), fov_axis)
    s = loaders.SceneLoadSettings(path=p, split_method=abi.SPLIT_MIDDLE, max_shapes_in_node=3)
    got = loaders.load_mitsuba(s)
    want = mr.load_mitsuba(p, abi.SPLIT_MIDDLE, 3)
    mr.assert_same_loaded(want, got)
    sd, cam, film = got
    assert film.res == (96, 64) and film.tile_dim == 16
    assert cam.fov_axis == (abi.FOV_X if fov_axis == "x" else abi.FOV_Y) and cam.fov_degrees == 42.5
    assert sd.n_triangles == 60 and sd.meshes == [(False, False, True), (True, True, True), (False, False, True), (True, False, True), (False, False, True)]
    assert (sd.split_method, sd.max_shapes_in_node) == (abi.SPLIT_MIDDLE, 3)
    # every bsdf element appends one record in document order; the second "grey" serves the later shapes only
    assert [m["kind"] for m in sd.materials] == [abi.MAT_MATTE] * 5 + [abi.MAT_GLASS] * 2 + [abi.MAT_MATTE]
    assert [int(sd.tri_material[12 * k]) for k in range(5)] == [0, 5, 2, 7, 3]
    assert sd.materials[1]["a"] == (0.5, 0.5, 0.5) and sd.materials[3]["a"][2] == 0.0 and sd.materials[4]["a"] == (1.0, 1.0, 1.0)
    assert np.float32(sd.materials[6]["c"]) == np.float32(1.5046) and np.float32(sd.materials[5]["c"]) == np.float32(1.33)
    assert np.array(sd.background, np.float32).tobytes() == np.array([0.15, 0.2, 0.3], np.float32).tobytes()  # the last constant emitter
    assert [l.kind for l in sd.light_structs] == [abi.LIGHT_POINT, abi.LIGHT_SPOT]
    assert tuple(sd.light_structs[0].p) == (2.5, 4.0, -1.5)  # x negated; attribute order x, z, y
    # float64 anchors from the file's numbers
    root = ET.parse(p).getroot()
    T = MIRROR @ _xf64(root.find("sensor/transform"))
    for loaded in (got, want):
        c = loaded[1]
        assert _close(c.position, T[:3, 3])
        d = np.array(c.target, np.float64) - np.array(c.position, np.float64)
        assert _close(d / np.linalg.norm(d), T[:3, 2])  # a Mitsuba sensor looks along its +Z
        assert _close(c.up, T[:3, 1])
        first = 0
        for shape in root.findall("shape"):
            fn = shape.find("string").get("value").replace("\\", "/")
            raw = ol._read_ply(os.path.join(str(tmp_path), fn))[0]
            t = shape.find("transform")
            M = MIRROR @ (_xf64(t) if t is not None else np.eye(4))
            for k in (0, len(raw) - 1):
                assert _close(loaded[0].points[first + k], (M @ np.array([*raw[k], 1.0], np.float64))[:3])
            first += len(raw)
        assert first == len(loaded[0].points)
    # the target sits in the middle of the scene's bounds along the view direction (mod.rs:192-203)
    lo, hi = sd.points.min(axis=0).astype(np.float64), sd.points.max(axis=0).astype(np.float64)
    o, d = np.array(cam.position, np.float64), T[:3, 2]
    t0, t1 = (lo - o) / d, (hi - o) / d
    p0, p1 = max(np.minimum(t0, t1).max(), 0.0), np.maximum(t0, t1).min()
    assert p0 > 0 and _close(cam.target, o + d * (p0 + p1) / 2)


# ----------------------------------------------------------------------------- quirks
def _both_reject(mr, path, fragment):
    with pytest.raises(mr.LoadError) as oe:
        mr.load_mitsuba(path)
    with pytest.raises(YukiError) as e:
        loaders.load_mitsuba(path)
    assert fragment in str(oe.value), str(oe.value)
    assert str(oe.value) in str(e.value), (str(oe.value), str(e.value))  # the same message: it names the same element
    return e.value


def _edit(text, old, new, count=1):
    assert text.count(old) >= 1, old
    return text.replace(old, new, count)


HAND = mf.HAND_XML % dict(fov_axis="x")

REJECTED = {
    "position_not_first_in_point": (lambda t: _edit(t, '<point name="position" x="-2.5"', '<point x="-2.5" name="position"'), "Invalid point axis 'name'"),
    "double_space_in_rgb": (lambda t: _edit(t, "60 55 50", "60  55 50"), "invalid float literal '' in element 'rgb intensity'"),
    "scale_with_two_numbers": (lambda t: _edit(t, '<scale value="12 0.5 8"/>', '<scale value="12 0.5"/>'), "scale needs one or three numbers"),
    "scale_with_four_numbers": (lambda t: _edit(t, '<scale value="12 0.5 8"/>', '<scale value="12 0.5 8 1"/>'), "scale needs one or three numbers"),
    "translate_with_two_numbers": (lambda t: _edit(t, '<translate value="-0.5 -1 -0.25"/>', '<translate value="-0.5 -1"/>'), "translate needs three numbers"),
    "matrix_with_15_numbers": (lambda t: _edit(t, "0 -0.5 2 0.5 0 0 0 1", "0 -0.5 2 0.5 0 0 0"), "matrix needs 16 numbers"),
    "rgb_with_four_components": (lambda t: _edit(t, "0.6 0.55 0.5", "0.6 0.55 0.5 1"), "rgb 'reflectance' has more than three components"),
    "ext_ior_of_water": (lambda t: _edit(t, 'value="1.0003"', 'value="1.33"'), "Only air supported for external IoR not supported but received '1.33"),
    "missing_fov_axis": (lambda t: _edit(t, '<string name="fov_axis" value="x"/>', ""), "Unknown fov axis ''"),
    "fov_axis_z": (lambda t: _edit(t, '<string name="fov_axis" value="x"/>', '<string name="fov_axis" value="z"/>'), "Unknown fov axis 'z'"),
    "camera_transform_with_scale": (lambda t: _edit(t, '<translate value="0.75 2.25 -6.5"/>', '<scale value="2"/><translate value="0.75 2.25 -6.5"/>'), "Camera to world has scaling"),
    "version_2_0_0": (lambda t: _edit(t, 'version="2.1.0"', 'version="2.0.0"'), "Scene file version is not 2.1.0"),
    "no_version": (lambda t: _edit(t, ' version="2.1.0"', ""), "Could not find element attribute 'version'"),
    "unknown_top_level_element": (lambda t: _edit(t, '<emitter type="constant">', '<texture type="bitmap"/><emitter type="constant">'), "Unknown element: 'texture'"),
    "text_between_tags": (lambda t: _edit(t, '<bsdf type="diffuse" id="half"/>', '<bsdf type="diffuse" id="half"/>hello<bsdf type="diffuse" id="h2"/>'), "Unexpected characters outside tags: hello"),
    "cdata": (lambda t: _edit(t, '<emitter type="constant">', "<![CDATA[x < y]]><emitter type=\"constant\">"), "Unexpected CDATA: x < y"),
    "processing_instruction": (lambda t: _edit(t, '<emitter type="constant">', "<?render fast?><emitter type=\"constant\">"), "Unexpected processing instruction: render"),
    "material_defined_after_its_shape": (lambda t: _edit(t, '<ref id="glass" name="bsdf"/>', '<ref id="late" name="bsdf"/>').replace("</scene>", '<bsdf type="diffuse" id="late"/></scene>'),
                                         "Unknown mesh material 'late'"),
    "dielectric_nested_in_twosided": (lambda t: _edit(t, '<bsdf type="twosided" id="two_bare"/>', '<bsdf type="twosided" id="two_bare"><bsdf type="dielectric"><float name="int_ior" value="1.5"/></bsdf></bsdf>'),
                                      "Unknown light data type 'float'"),
    "unknown_bsdf_type": (lambda t: _edit(t, '<bsdf type="diffuse" id="half"/>', '<bsdf type="plastic" id="half"/>'), "Unknown bsdf type 'plastic'"),
    "sphere_shape": (lambda t: _edit(t, '<shape type="ply">', '<shape type="sphere">'), "Unexpected shape type 'sphere'!"),
    "shape_without_ref": (lambda t: _edit(t, '<ref name="bsdf" id="two_nested"/>', ""), "Mesh with no material"),
    "shape_without_filename": (lambda t: _edit(t, '<string name="filename" value="geo/cube_le.ply"/>', ""), "Mesh with no ply"),
    "resx_not_u16": (lambda t: _edit(t, 'name="resx" value="96"', 'name="resx" value="65536"'), "invalid integer '65536' in element 'default resx'"),
    "hex_float": (lambda t: _edit(t, 'name="fov" value="42.5"', 'name="fov" value="0x2A"'), "invalid float literal '0x2A' in element 'float fov'"),
    "padded_float": (lambda t: _edit(t, 'name="fov" value="42.5"', 'name="fov" value=" 42.5"'), "invalid float literal ' 42.5' in element 'float fov'"),
    "unknown_sensor_float": (lambda t: _edit(t, 'name="near_clip"', 'name="aperture"'), "Unknown sensor string element 'aperture'"),
    "unknown_transform_child": (lambda t: _edit(t, '<scale value="4"/>', '<lookat origin="0 0 0" target="0 0 1" up="0 1 0"/>'), "Unknown transformation data type 'lookat'"),
    "spot_float_of_another_name": (lambda t: _edit(t, 'name="beam_width"', 'name="falloff"'), "Unexpected spot light float 'name': 'falloff'"),
    "dielectric_rgb_of_another_name": (lambda t: _edit(t, 'name="specular_transmittance"', 'name="tint"'), "Unknown dielectric rgb data 'tint'"),
    # item 9: the first failure in DOCUMENT order wins
    "missing_ply_before_a_later_unknown_element": (lambda t: _edit(t, 'value="geo/cube_le.ply"', 'value="geo/missing.ply"').replace("</scene>", "<texture/></scene>"), "Could not open '"),
    "unknown_element_before_a_later_missing_ply": (lambda t: _edit(t, '<bsdf type="diffuse" id="grey">\n    <rgb name="reflectance" value="0.1', '<texture/><bsdf type="diffuse" id="grey">\n    <rgb name="reflectance" value="0.1')
                                                   .replace('value="geo/cube_le.ply"', 'value="geo/missing.ply"'), "Unknown element: 'texture'"),
    # item 10: the element in progress is completed from the children read so far
    "file_ends_in_a_shape_before_its_ref": (lambda t: t[: t.index('<ref name="bsdf" id="two_direct"/>')], "Mesh with no material"),
    "repeated_attribute_on_a_ref": (lambda t: _edit(t, '<ref name="bsdf" id="two_direct"/>', '<ref name="bsdf" id="two_direct" id="grey"/>'), "Mesh with no material"),
    "file_ends_before_the_first_shape": (lambda t: t[: t.index("<shape")], "scene has no shapes"),
}


@pytest.mark.parametrize("case", sorted(REJECTED))
def test_quirk_rejected_by_both(tmp_path, mr, case):
    edit, fragment = REJECTED[case]
    p = mf.write_hand_scene(str(tmp_path), text=edit(HAND))
    e = _both_reject(mr, p, fragment)
    assert e.status != 0


def test_doctype_is_unsupported(tmp_path, mr):
    p = mf.write_hand_scene(str(tmp_path), text=HAND.replace("<scene", '<!DOCTYPE scene SYSTEM "scene.dtd">\n<scene', 1))
    with pytest.raises(mr.Unsupported):
        mr.load_mitsuba(p)
    with pytest.raises(YukiError) as e:
        loaders.load_mitsuba(p)
    assert e.value.status == ERR_UNSUPPORTED and "DOCTYPE" in str(e.value)


def test_broken_ply_is_reported_before_a_later_unknown_element(tmp_path, mr):
    """The reference loads each PLY inside shape::parse, so a PLY that does not load comes before anything later in the
    document, the opposite of the pbrt loader (tests/test_loaders.py::test_pbrt_parse_error_after_a_broken_ply_wins)."""
    text = HAND.replace('value="geo/cube_le.ply"', 'value="geo/bad.ply"').replace("</scene>", "<texture/></scene>")
    p = mf.write_hand_scene(str(tmp_path), text=text)
    (tmp_path / "geo" / "bad.ply").write_bytes(b"ply\nformat ascii 1.0\nelement vertex 1\nproperty float x\nend_header\n0\n")
    with pytest.raises(mr.LoadError) as oe:
        mr.load_mitsuba(p)
    with pytest.raises(YukiError) as e:
        loaders.load_mitsuba(p)
    assert "PLY" in str(oe.value) and "PLY" in str(e.value) and "texture" not in str(e.value)
    for threads in ("1", "3"):  # whichever thread reads the files, the error is the sequential order's
        os.environ["YK_LOADER_THREADS"] = threads
        try:
            with pytest.raises(YukiError) as e2:
                loaders.load_mitsuba(p)
        finally:
            del os.environ["YK_LOADER_THREADS"]
        assert str(e2.value) == str(e.value)


def test_filename_with_back_slashes(tmp_path, mr):
    p = mf.write_hand_scene(str(tmp_path))
    assert 'value="geo\\cube_be.ply"' in open(p).read()
    sd, _, _ = loaders.load_mitsuba(p)
    assert len(sd.meshes) == 5 and sd.meshes[2] == (False, False, True)


MALFORMED = {
    # the file ends inside the fourth shape, after its filename and ref but before its transform: the shape is completed without one
    "file_ends_inside_an_element": (lambda t: t[: t.index('<transform name="to_world">\n      <scale value="3 3 3"/>')].replace('value="geo/cube_n.ply"/>', 'value="geo/cube_n.ply"/><ref name="bsdf" id="half"/>'), 4),
    "end_tag_that_does_not_match": (lambda t: _edit(t, '<ref name="bsdf" id="grey"/>\n  </shape>\n  <shape type="ply">\n    <string name="filename" value="cube.ply"/>',
                                                    '<ref name="bsdf" id="grey"/>\n  </shap>\n  <shape type="ply">\n    <string name="filename" value="cube.ply"/>'), 4),
    "repeated_attribute": (lambda t: _edit(t, '<shape type="ply">\n    <string name="filename" value="cube.ply"/>\n    <transform name="to_world">\n      <scale value="0.75"/>',
                                           '<shape type="ply" type="ply">\n    <string name="filename" value="cube.ply"/>\n    <transform name="to_world">\n      <scale value="0.75"/>'), 4),
}


@pytest.mark.parametrize("case", sorted(MALFORMED))
def test_malformed_xml_loads_what_came_before(tmp_path, mr, case):
    """mod.rs:179-182, macros.rs:100-103: an XML error is logged and reading stops; the scene is built from what was read."""
    edit, n_meshes = MALFORMED[case]
    text = edit(HAND)
    assert text != HAND
    p = mf.write_hand_scene(str(tmp_path), text=text)
    got = loaders.load_mitsuba(p)
    want = mr.load_mitsuba(p)
    mr.assert_same_loaded(want, got)
    assert len(got[0].meshes) == n_meshes and got[0].n_triangles == 12 * n_meshes
    if case == "file_ends_inside_an_element":  # no transform was read: the mirror alone
        raw = np.array([c * 0.3 for c in sf.CUBE_V[0]], dtype=np.float32)
        assert got[0].points[24][0] == -raw[0] and got[0].points[24][1] == raw[1]


# ----------------------------------------------------------------------------- round trip
def _round_trip(tmp_path, mr, sd, **kw):
    p, written, info = mf.write_scene_as_mitsuba(sd, str(tmp_path), **kw)
    got = loaders.load_mitsuba(p)
    want = mr.load_mitsuba(p)
    mr.assert_same_loaded(want, got)
    g = got[0]
    assert np.array_equal(g.points, sd.points) and np.array_equal(g.indices, written.indices)
    assert kw.get("reverse_winding") or np.array_equal(g.indices, sd.indices)
    assert (g.uvs is None and not any(m[1] for m in sd.meshes)) or np.array_equal(g.uvs, sd.uvs)
    assert g.meshes == written.meshes and all(m[2] for m in g.meshes)
    assert np.array_equal(g.tri_mesh, sd.tri_mesh) and np.array_equal(g.tri_material, written.tri_material)
    assert np.all(g.tri_area_light == -1)
    assert len(g.materials) == len(written.materials)
    for a, b in zip(g.materials, written.materials):
        assert a["kind"] == b["kind"] and np.array_equal(np.float32(a["a"]), np.float32(b["a"])) and np.array_equal(np.float32(a["b"]), np.float32(b["b"])) and np.float32(a["c"]) == np.float32(b["c"])
    assert len(g.light_structs) == info["lights"]
    assert np.array_equal(np.float32(g.background), np.float32(sd.background))
    return got, written


@pytest.mark.parametrize("reverse_winding", [False, True])
def test_round_trip_city_small(tmp_path, mr, reverse_winding):
    """reverse_winding (what the GPU tests render, tests/mitsuba_files.py): the faces come back as (i0, i2, i1), so that the
    flip of the geometric normal on a mirrored mesh (shapes/triangle.rs:187-194) restores the generator's normals."""
    from yuki_amd import scenes

    sd = scenes.by_name("city-small")
    (g, cam, film), written = _round_trip(tmp_path, mr, sd, res=(320, 180), reverse_winding=reverse_winding)
    assert np.array_equal(g.indices, sd.indices[:, [0, 2, 1]] if reverse_winding else sd.indices)
    assert film.res == (320, 180) and len(g.meshes) == 26 and len(g.light_structs) == 2  # the area light is dropped, as for the pbrt variant
    kinds = {m["kind"] for m in sd.materials}
    assert len(kinds) > 2 and {m["kind"] for m in g.materials} == {abi.MAT_MATTE, abi.MAT_GLASS}  # the "mixed" city becomes matte and glass
    assert np.allclose(cam.position, sd.camera["position"], rtol=1e-6, atol=1e-6)
    d0 = np.subtract(sd.camera["target"], sd.camera["position"])
    d1 = np.subtract(cam.target, cam.position)
    assert np.allclose(d0 / np.linalg.norm(d0), d1 / np.linalg.norm(d1), atol=1e-5)


def test_round_trip_cfg2_mesh(tmp_path, mr):
    from yuki_amd import scenes

    sd = scenes.by_name("cfg2")
    (g, cam, film), written = _round_trip(tmp_path, mr, sd, twosided=True)
    assert g.n_triangles == 69312 and g.meshes == [(False, False, True)] and film.res == (1920, 1080)
    assert len(g.light_structs) == 1 and g.light_structs[0].kind == abi.LIGHT_POINT and tuple(g.light_structs[0].p) == (5.0, 5.0, 0.0)


# ----------------------------------------------------------------------------- dispatch
def test_load_scene_dispatches_by_extension(tmp_path, mr):
    xml = mf.write_hand_scene(str(tmp_path))
    pbrt = sf.write_scene(str(tmp_path / "pbrt"))
    ply = str(tmp_path / "cube.ply")
    for path, direct in ((xml, loaders.load_mitsuba), (pbrt, loaders.load_pbrt), (ply, loaders.load_ply)):
        a, b = loaders.load_scene(path), direct(path)
        assert a[1] == b[1] and a[2] == b[2]
        assert a[0].points.tobytes() == b[0].points.tobytes() and a[0].indices.tobytes() == b[0].indices.tobytes()
        assert a[0].materials == b[0].materials and [bytes(x) for x in a[0].light_structs] == [bytes(x) for x in b[0].light_structs]
    s = loaders.SceneLoadSettings(path=xml, split_method=abi.SPLIT_MIDDLE, max_shapes_in_node=2)
    assert (loaders.load_scene(s)[0].split_method, loaders.load_scene(s)[0].max_shapes_in_node) == (abi.SPLIT_MIDDLE, 2)
    upper = str(tmp_path / "scene.XML")
    os.replace(xml, upper)
    (tmp_path / "noext").write_text("x")
    (tmp_path / ".xml").write_text("x")
    for path, message in ((upper, "Unknown extension 'XML'"), (str(tmp_path / "noext"), "Expected a file with an extension"), (str(tmp_path / ".xml"), "Expected a file with an extension"),
                          (str(tmp_path / "missing.xml"), "Scene does not exist '%s'" % (tmp_path / "missing.xml")), ("", "")):
        with pytest.raises(YukiError) as e:
            loaders.load_scene(path)
        assert e.value.status == ERR_INVALID_ARGUMENT and message in str(e.value), (path, str(e.value))


# ----------------------------------------------------------------------------- load time at BASELINE size
@pytest.fixture(scope="session")
def cfg3_files(tmp_path_factory, cfg3_scene):
    """cfg3 as scene.pbrt + 802 PLY files, and scene.xml beside it naming the same PLY files (it loads mirrored)."""
    d = str(tmp_path_factory.mktemp("cfg3_mitsuba"))
    pbrt, info = sf.write_scene_as_pbrt(d, cfg3_scene)
    assert info["ply_files"] == 802
    spot = dict(kind="spot", cutoff=40.0, beam=30.0, I=(400.0, 380.0, 350.0), transform='<rotate x="1" angle="80"/><rotate y="1" angle="30"/><translate value="-20 4 10"/>')
    xml, written, info = mf.write_scene_as_mitsuba(cfg3_scene, d, extra_lights=[spot], reuse_meshes=True)
    assert info["shapes"] == 802 and info["ply_files"] == 0
    return pbrt, xml


@pytest.fixture(scope="session")
def cfg3_checker_loaded(cfg3_files, oracle):
    """tests/mitsuba_ref.py on the 1,024,012-triangle file set: per-vertex Python through the oracle's transforms."""
    import mitsuba_ref

    return mitsuba_ref.load_mitsuba(cfg3_files[1])


def test_cfg3_load_time_and_fields(cfg3_files, cfg3_checker_loaded, cfg3_scene, mr):
    """802 PLY shapes, 1,024,012 triangles: yk_load_mitsuba takes no more than 1.5 x the time yk_load_pbrt needs for its variant of
    the same scene (best of three each, after one untimed call); the XML is a few hundred KB beside 36 MB of PLY, the 50 % is
    for a shared host's noise on a 0.1-0.4 s measurement.  Measured: see DESIGN.md section 2."""
    pbrt, xml = cfg3_files

    def best(fn, path):
        fn(path)
        ts = []
        for _ in range(3):
            t0 = time.perf_counter()
            out = fn(path)
            ts.append(time.perf_counter() - t0)
        return min(ts), out

    t_pbrt, _ = best(loaders.load_pbrt, pbrt)
    t_xml, got = best(loaders.load_mitsuba, xml)
    print(f"cfg3 files: yk_load_pbrt {t_pbrt:.3f} s, yk_load_mitsuba {t_xml:.3f} s (best of three, {os.path.getsize(xml) / 1e3:.0f} KB of XML)")
    mr.assert_same_loaded(cfg3_checker_loaded, got)
    g = got[0]
    assert g.n_triangles == 1024012 and len(g.meshes) == 802 and all(m[2] for m in g.meshes) and len(g.light_structs) == 3
    assert np.array_equal(g.points * np.float32([-1, 1, 1]), cfg3_scene.points) and np.array_equal(g.indices, cfg3_scene.indices)
    assert t_xml <= 1.5 * t_pbrt, (t_xml, t_pbrt)


# ----------------------------------------------------------------------------- the reference's constants and names
REFERENCE_MITSUBA = os.path.join(os.environ.get("YUKI_REFERENCE", "/root/reference"), "yuki", "src", "scene", "mitsuba")
RS_FILES = ("mod.rs", "sensor.rs", "transform.rs", "shape.rs", "material.rs", "emitter.rs", "common.rs")


def _reference_facts():
    """Read out of scene/mitsuba/*.rs (nothing is stored): the version string, the IoR constants and their tolerance, the default
    reflectance, the string literals each parser's `match` arms name and the attributes it asks for."""
    src = {n: open(os.path.join(REFERENCE_MITSUBA, n)).read() for n in RS_FILES}
    f = lambda text: float(text.replace("_", ""))  # noqa: E731
    facts = dict(
        version=re.search(r'"version"\)\.as_str\(\) != "([^"]+)"', src["mod.rs"]).group(1),
        bk7=f(re.search(r"const BK7_GLASS_IOR: f32 = ([\d._]+);", src["material.rs"]).group(1)),
        air=f(re.search(r"const AIR_IOR: f32 = ([\d._]+);", src["material.rs"]).group(1)),
        eps=f(re.search(r"abs_diff_eq!\(ext_ior, AIR_IOR, epsilon = ([\d._]+)\)", src["material.rs"]).group(1)),
        reflectance=[f(v) for v in re.search(r"fn parse_diffuse.*?Spectrum::new\(([\d._]+), ([\d._]+), ([\d._]+)\)", src["material.rs"], re.S).groups()],
        arms={}, attrs={},
    )
    for n, text in src.items():
        arms = re.findall(r'^\s*((?:"[^"]*"\s*\|\s*)*"[^"]*")\s*=>', text, re.M)
        facts["arms"][n] = sorted({s for a in arms for s in re.findall(r'"([^"]*)"', a)})
        facts["attrs"][n] = sorted(set(re.findall(r'find_attr!\(\s*&?attributes,\s*"(\w+)"\s*\)', text)))
    return facts


# what yk_mitsuba.cpp matches on, file by file (element names, `type` / `name` values, point axes)
PRODUCT_ARMS = {
    "mod.rs": ["bsdf", "default", "dielectric", "diffuse", "emitter", "integrator", "resx", "resy", "scene", "sensor", "shape", "twosided"],
    "sensor.rs": ["", "far_clip", "film", "float", "fov", "fov_axis", "near_clip", "sampler", "string", "transform", "x", "y"],
    "transform.rs": ["matrix", "rotate", "scale", "translate"],
    "shape.rs": ["ref", "string", "transform"],
    "material.rs": ["bsdf", "ext_ior", "float", "int_ior", "rgb"],
    "emitter.rs": ["beam_width", "constant", "cutoff_angle", "float", "point", "rgb", "spot", "transform", "x", "y", "z"],
    "common.rs": [],
}
PRODUCT_ATTRS = {"mod.rs": ["id", "name", "type", "value", "version"], "sensor.rs": ["name", "value"], "transform.rs": ["angle", "value", "x", "y", "z"], "shape.rs": ["id", "name", "type", "value"],
                 "material.rs": ["name", "value"], "emitter.rs": ["name", "type", "value"], "common.rs": ["name", "value"]}
BARE = """<scene version="%(version)s">%(top)s<sensor><string name="fov_axis" value="x"/>%(sensor)s<transform>%(transform)s</transform></sensor>
<bsdf type="diffuse" id="d"/><bsdf type="dielectric" id="g">%(dielectric)s</bsdf>
<shape type="ply"><string name="filename" value="cube.ply"/><ref name="bsdf" id="d"/>%(shape)s</shape>
<shape type="ply"><string name="filename" value="cube.ply"/><ref name="bsdf" id="g"/></shape></scene>"""


def _check_reference_facts(facts, tmp):
    """Compare the facts with what the product accepts for bare elements; returns the list of differences."""
    problems = []

    def load(**kw):
        args = dict(version=facts["version"], top="", sensor="", transform="", dielectric="", shape="")
        args.update(kw)
        p = mf.write_hand_scene(tmp, text=BARE % args)
        try:
            return loaders.load_mitsuba(p)[0], ""
        except YukiError as e:
            return None, str(e)

    sd, err = load()
    if sd is None:
        return ["version '%s' is refused: %s" % (facts["version"], err)]
    if np.float32(sd.materials[1]["c"]) != np.float32(facts["bk7"]):
        problems.append("default int_ior %r != %r" % (sd.materials[1]["c"], facts["bk7"]))
    if [np.float32(v) for v in sd.materials[0]["a"]] != [np.float32(v) for v in facts["reflectance"]]:
        problems.append("default reflectance %r != %r" % (sd.materials[0]["a"], facts["reflectance"]))
    for k, accepted in ((0.0, True), (0.9, True), (-0.9, True), (1.1, False), (-1.1, False)):
        ior = "%.9g" % (facts["air"] + k * facts["eps"])
        if (load(dielectric='<float name="ext_ior" value="%s"/>' % ior)[0] is not None) != accepted:
            problems.append("ext_ior %s should be %s" % (ior, "accepted" if accepted else "refused"))
    # element names: a parser that knows a name does not answer `Unknown ... 'name'`
    probes = {"mod.rs": "top", "sensor.rs": "sensor", "transform.rs": "transform", "shape.rs": "shape"}
    elements = {"mod.rs": {"scene", "default", "integrator", "sensor", "bsdf", "emitter", "shape"}, "sensor.rs": {"string", "float", "transform", "sampler", "film"},
                "transform.rs": {"rotate", "translate", "scale", "matrix"}, "shape.rs": {"string", "ref", "transform"}}
    pool = set().union(*elements.values()) | {"lookat", "texture"}
    for n, slot in probes.items():
        for name in sorted(pool):
            _, err = load(**{slot: "<%s/>" % name})
            if name in facts["arms"][n] and name not in elements[n]:
                continue  # an arm of this file that matches a `type` / `name` value ("point", "float" in emitter.rs ...), not an element here
            known = not ("Unknown" in err and "'%s'" % name in err)
            if known != (name in facts["arms"][n]):
                problems.append("%s: element '%s' is %s by the library" % (n, name, "known" if known else "unknown"))
    for n in RS_FILES:
        if facts["arms"][n] != PRODUCT_ARMS[n]:
            problems.append("%s: match arms %r != %r" % (n, facts["arms"][n], PRODUCT_ARMS[n]))
        if facts["attrs"][n] != PRODUCT_ATTRS[n]:
            problems.append("%s: attributes %r != %r" % (n, facts["attrs"][n], PRODUCT_ATTRS[n]))
    return problems


needs_reference = pytest.mark.skipif(not os.path.isdir(REFERENCE_MITSUBA), reason="the reference's source tree is not on this machine")


@needs_reference
def test_reference_constants_and_names(tmp_path):
    facts = _reference_facts()
    assert facts["version"] == "2.1.0" and len(facts["arms"]["mod.rs"]) == 12
    assert _check_reference_facts(facts, str(tmp_path)) == []


@needs_reference
@pytest.mark.parametrize("what", ["version", "bk7", "air", "eps", "reflectance", "arm", "attr", "element"])
def test_the_check_sees_a_changed_reference_constant(tmp_path, what):
    """The comparison is not vacuous: one changed constant of each kind is reported."""
    facts = _reference_facts()
    if what == "version":
        facts["version"] = "2.1.1"
    elif what == "bk7":
        facts["bk7"] = float(np.nextafter(np.float32(facts["bk7"]), np.float32(2)))
    elif what == "air":
        facts["air"] += 0.0005
    elif what == "eps":
        facts["eps"] *= 1.5
    elif what == "reflectance":
        facts["reflectance"][1] = 0.4
    elif what == "arm":
        facts["arms"]["emitter.rs"] = sorted(facts["arms"]["emitter.rs"] + ["area"])
    elif what == "attr":
        facts["attrs"]["transform.rs"] = sorted(facts["attrs"]["transform.rs"] + ["origin"])
    else:
        facts["arms"]["transform.rs"] = sorted(facts["arms"]["transform.rs"] + ["lookat"])
    assert _check_reference_facts(facts, str(tmp_path)), what
