"""TEST INFRASTRUCTURE ONLY — a second, independent reading of the reference's Mitsuba 2.1.0 loader
(yuki/src/scene/mitsuba/{mod,macros,sensor,shape,material,emitter,transform,common}.rs), against which
yuki_amd/csrc/yk_mitsuba.cpp is compared bit for bit.

Independent where it can be: the XML events come from Python's expat binding (the product has a hand-written
reader), numbers are numpy float32, and every piece of arithmetic goes through the oracle's KAT-pinned
restatement of the reference's math (oracle.binding: orc_rotation_f32, orc_mat4_mul_f32, orc_mat4_inverse_f32,
orc_transform_apply_f32, orc_sinf / orc_cosf / orc_atan2f, orc_slab_test_f32, orc_make_spot_light /
orc_make_point_light) and oracle/loaders.py's PLY reader and Transform helpers.

Parity unpinned: the reference holds no tests, fixtures or sample files for this loader and its XML crate
(xml-rs) is not part of its tree; both sides follow the source text.  On a well-formedness error the reference
logs and stops reading, every nesting level finishing with what it has (mod.rs:179-182, macros.rs:100-103);
that is restated here with expat's error as the stop.
"""
import ctypes as C
import os
import re
from xml.parsers import expat

import numpy as np

from oracle import binding
from oracle import loaders as ol
from yuki_amd import abi
from yuki_amd.core import CameraParameters, FilmSettings

F = np.float32
LoadError = ol.LoadError


class Unsupported(LoadError):
    pass


# ------------------------------------------------------------------ events
_WS = " \t\r\n"


def xml_events(data):
    """[('start', name, [(attr, value), ...]) | ('end', name) | ('chars', text) | ('cdata', text) | ('pi', target) |
    ('doctype',)] + one closing ('enddoc',) or ('error',).  White-space-only character data is dropped (XmlEvent::Whitespace)."""
    out, text, cdata = [], [], [None]

    def flush():
        if text:
            s = "".join(text)
            del text[:]
            if s.strip(_WS):
                out.append(("chars", s))

    def start(name, attrs):
        flush()
        out.append(("start", name, [(attrs[i], attrs[i + 1]) for i in range(0, len(attrs), 2)]))

    def end(name):
        flush()
        out.append(("end", name))

    def chars(s):
        (cdata[0] if cdata[0] is not None else text).append(s)

    def cdata_start():
        flush()
        cdata[0] = []

    def cdata_end():
        out.append(("cdata", "".join(cdata[0])))
        cdata[0] = None

    def pi(target, _data):
        flush()
        out.append(("pi", target))

    class _Doctype(Exception):
        pass

    def doctype(*_a):
        flush()
        out.append(("doctype",))
        raise _Doctype()

    p = expat.ParserCreate()
    p.ordered_attributes = True
    p.buffer_text = False
    p.StartElementHandler, p.EndElementHandler, p.CharacterDataHandler = start, end, chars
    p.StartCdataSectionHandler, p.EndCdataSectionHandler = cdata_start, cdata_end
    p.ProcessingInstructionHandler, p.StartDoctypeDeclHandler = pi, doctype
    try:
        p.Parse(data, True)
        flush()
        out.append(("enddoc",))
    except _Doctype:
        pass
    except expat.ExpatError:
        flush()
        out.append(("error",))
    return out


class _Reader:
    """parser.next(): an error (and the end of the document) is returned again on every later call."""

    def __init__(self, events):
        self.ev, self.i = events, 0

    def next(self):
        e = self.ev[min(self.i, len(self.ev) - 1)]
        self.i += 1
        return e


# ------------------------------------------------------------------ attributes and numbers
_FLOAT = re.compile(r"[+-]?(?:(?i:inf|infinity|nan)|(?:[0-9]+\.?[0-9]*|\.[0-9]+)(?:[eE][+-]?[0-9]+)?)")
_U16 = re.compile(r"\+?[0-9]+")


def try_find_attr(attrs, name):  # macros.rs:2-12: the last one of that name
    v = None
    for n, val in attrs:
        if n == name:
            v = val
    return v


def find_attr(attrs, name):  # macros.rs:15-22
    v = try_find_attr(attrs, name)
    if v is None:
        raise LoadError(f"Could not find element attribute '{name}'")
    return v


def parse_f32(v, element):
    """str::parse::<f32>: Rust's grammar, correctly rounded straight to binary32."""
    if not _FLOAT.fullmatch(v):
        raise LoadError(f"invalid float literal '{v}' in element '{element}'")
    return F(ol._libc.strtof(v.encode(), None))


def parse_u16(v, element):
    if not _U16.fullmatch(v) or int(v) > 65535:
        raise LoadError(f"invalid integer '{v}' in element '{element}'")
    return int(v)


def parse_list(v, element):
    return [parse_f32(piece, element) for piece in v.split(" ")]


def parse_rgb(attrs, expected):  # common.rs:4-18
    name = find_attr(attrs, "name")
    if name != expected:
        raise LoadError(f"Expected rgb to be '{expected}', got '{name}'")
    c = parse_list(find_attr(attrs, "value"), f"rgb {expected}")
    if len(c) > 3:
        raise LoadError(f"rgb '{expected}' has more than three components")
    return tuple(c + [F(0)] * (3 - len(c)))


# ------------------------------------------------------------------ parse_element! (macros.rs:32-107)
class _State:
    def __init__(self):
        self.level = 0
        self.ignore = None


def _unexpected(e):
    if e[0] == "pi":
        raise LoadError(f"Unexpected processing instruction: {e[1]}")
    if e[0] == "cdata":
        raise LoadError(f"Unexpected CDATA: {e[1]}")
    if e[0] == "chars":
        raise LoadError(f"Unexpected characters outside tags: {e[1]}")
    if e[0] == "doctype":
        raise Unsupported("DOCTYPE declarations are not supported")


def parse_element(rd, body):
    st = _State()
    while True:
        e = rd.next()
        if e[0] == "start":
            if st.ignore is None:
                body(e[1], e[2], st)
            st.level += 1
            if st.ignore is not None:
                st.ignore += 1
        elif e[0] == "end":
            if st.ignore is not None:
                after = st.ignore - 1
                st.ignore = after if after > 0 else None
            st.level -= 1
            if st.level < 0:
                return
        elif e[0] in ("error", "enddoc"):
            return
        else:
            _unexpected(e)


# ------------------------------------------------------------------ math through the oracle
def _inverse(m):
    out = np.zeros(16, dtype=F)
    binding.lib().orc_mat4_inverse_f32(binding._p(np.ascontiguousarray(m, dtype=F).reshape(16)), binding._p(out))
    return out


def _axis_rotation(axis, theta):  # rotation_x / _y / _z
    m, mi = np.zeros(16, dtype=F), np.zeros(16, dtype=F)
    binding.lib().orc_rotation_f32(axis, C.c_float(float(theta)), binding._p(np.zeros(3, dtype=F)), binding._p(m), binding._p(mi))
    return ol.Xf(m, mi)


def _len(v):
    out = np.zeros(9, dtype=F)
    a = np.ascontiguousarray(v, dtype=F)
    binding.lib().orc_vec3_ops_f32(binding._p(a), binding._p(a), binding._p(out))
    return F(out[4])


def _relative_eq(a, b):  # approx::relative_eq!, f32 defaults
    a, b = F(a), F(b)
    if a == b:
        return True
    if np.isinf(a) or np.isinf(b):
        return False
    eps = np.finfo(F).eps
    d = np.abs(a - b)
    if d <= eps:
        return True
    return bool(d <= max(np.abs(a), np.abs(b)) * eps)


def parse_transform(rd):  # transform.rs:14-81
    box = [ol.Xf()]

    def body(name, attrs, st):
        if name == "rotate":
            axis = [F(0), F(0), F(0)]
            for k, a in enumerate("xyz"):
                v = try_find_attr(attrs, a)
                if v is not None:
                    axis[k] = parse_f32(v, "rotate")
            with np.errstate(all="ignore"):
                axis = ol.normalized(axis)
                angle = parse_f32(find_attr(attrs, "angle"), "rotate") * ol.RADS_PER_DEG
            box[0] = ol.rotation(angle, axis) * box[0]
        elif name == "translate":
            p = parse_list(find_attr(attrs, "value"), "translate")
            if len(p) < 3:
                raise LoadError("translate needs three numbers")
            box[0] = ol.translation(p[:3]) * box[0]
        elif name == "scale":
            v = find_attr(attrs, "value")
            n = len(v.split(" "))
            if n not in (1, 3):
                raise LoadError("scale needs one or three numbers")
            p = parse_list(v, "scale")
            if n == 1:
                p = p * 3
            with np.errstate(all="ignore"):
                box[0] = ol.scale(*p) * box[0]
        elif name == "matrix":
            m = parse_list(find_attr(attrs, "value"), "matrix")
            if len(m) != 16:
                raise LoadError("matrix needs 16 numbers")
            mi = _inverse(m)
            if not np.all(np.isfinite(mi)):
                raise LoadError("matrix is singular")
            box[0] = ol.Xf(m, mi) * box[0]
        else:
            raise LoadError(f"Unknown transformation data type '{name}'")

    parse_element(rd, body)
    return box[0]


def parse_sensor(rd):  # sensor.rs:18-109
    s = dict(axis="", fov=F(0), xf=ol.Xf())

    def body(name, attrs, st):
        if name == "string":
            n, v = find_attr(attrs, "name"), find_attr(attrs, "value")
            if n != "fov_axis":
                raise LoadError(f"Unknown sensor string element '{n}'")
            s["axis"] = v
        elif name == "float":
            n, v = find_attr(attrs, "name"), find_attr(attrs, "value")
            if n == "fov":
                s["fov"] = parse_f32(v, "float fov")
            elif n not in ("near_clip", "far_clip", ""):
                raise LoadError(f"Unknown sensor string element '{n}'")
        elif name == "transform":
            s["xf"] = parse_transform(rd)
            st.level -= 1
        elif name in ("sampler", "film"):
            st.ignore = 0
        else:
            raise LoadError(f"Unknown sensor data type '{name}'")

    parse_element(rd, body)
    L = binding.lib()
    with np.errstate(all="ignore"):
        xf = ol.scale(-1.0, 1.0, 1.0) * s["xf"]
        m = xf.m
        position = (m[0, 3], m[1, 3], m[2, 3])
        sc = [_len(m[:3, k]) for k in range(3)]  # Matrix4x4::decompose, matrix.rs:218-255
        if any(v == 0 for v in sc):
            raise LoadError("Cannot decompose camera to world matrix: Cannot decompose matrix with a zero scale component")
        mr = [[m[r, c] / sc[c] for c in range(3)] for r in range(3)]
        tx = F(L.orc_atan2f(mr[1][2], mr[2][2]))
        c2 = np.sqrt(mr[0][0] * mr[0][0] + mr[0][1] * mr[0][1])
        ty = F(L.orc_atan2f(-mr[0][2], c2))
        s1, c1 = F(L.orc_sinf(tx)), F(L.orc_cosf(tx))
        tz = F(L.orc_atan2f(s1 * mr[2][0] - c1 * mr[1][0], c1 * mr[1][1] - s1 * mr[2][1]))
        if not all(_relative_eq(v, 1.0) for v in sc):
            raise LoadError("Camera to world has scaling")
        if s["axis"] not in ("x", "y"):
            raise LoadError("Unknown fov axis '%s'" % s["axis"])
        c2w = ol.translation(position) * (_axis_rotation(0, -tx) * (_axis_rotation(1, -ty) * _axis_rotation(2, tz)))
        target = c2w.apply(1, [0.0, 0.0, 1.0])
        up = c2w.apply(0, [0.0, 1.0, 0.0])
    return dict(position=tuple(F(v) for v in position), target=tuple(target), up=tuple(up), fov_axis=abi.FOV_X if s["axis"] == "x" else abi.FOV_Y, fov_degrees=s["fov"])


def _matte(rgb):
    return dict(kind=abi.MAT_MATTE, a=tuple(rgb), b=(0.0, 0.0, 0.0), c=0.0, remap=False)


def parse_diffuse(rd):  # material.rs:51-77
    box = [(F(0.5), F(0.5), F(0.5))]

    def body(name, attrs, st):
        if name != "rgb":
            raise LoadError(f"Unknown light data type '{name}'")
        box[0] = parse_rgb(attrs, "reflectance")

    parse_element(rd, body)
    return _matte(box[0])


def parse_twosided(rd):  # material.rs:17-49
    box = [_matte((F(1), F(1), F(1)))]

    def body(name, attrs, st):
        if name == "bsdf":
            box[0] = parse_diffuse(rd)
            st.level -= 1
        elif name == "rgb":
            box[0] = _matte(parse_rgb(attrs, "reflectance"))
        else:
            raise LoadError(f"Unknown material data type '{name}'")

    parse_element(rd, body)
    return box[0]


BK7_GLASS_IOR, AIR_IOR, EXT_IOR_EPSILON = F(1.5046), F(1.000277), F(0.001)


def parse_dielectric(rd):  # material.rs:79-142
    s = dict(int_ior=BK7_GLASS_IOR, ext_ior=AIR_IOR, r=(F(1),) * 3, t=(F(1),) * 3)

    def body(name, attrs, st):
        if name == "rgb":
            for key, expected in (("r", "specular_reflectance"), ("t", "specular_transmittance")):
                # `if let Ok(v) = parse_rgb(..)`: the name and the presence of a value decide; a bad number panics
                if try_find_attr(attrs, "name") == expected and try_find_attr(attrs, "value") is not None:
                    s[key] = parse_rgb(attrs, expected)
                    return
            raise LoadError("Unknown dielectric rgb data '%s'" % find_attr(attrs, "name"))
        elif name == "float":
            n = find_attr(attrs, "name")
            v = parse_f32(find_attr(attrs, "value"), "float " + n)
            if n == "int_ior":
                s["int_ior"] = v
            elif n == "ext_ior":
                s["ext_ior"] = v
            else:
                raise LoadError(f"Unknown dielectric float data '{n}'")
        else:
            raise LoadError(f"Unknown dielectric data type '{name}'")

    parse_element(rd, body)
    with np.errstate(all="ignore"):
        if not (np.abs(s["ext_ior"] - AIR_IOR) <= EXT_IOR_EPSILON):
            raise LoadError("Only air supported for external IoR not supported but received '%s'" % np.format_float_positional(s["ext_ior"], unique=True, trim="-"))
    return dict(kind=abi.MAT_GLASS, a=s["r"], b=s["t"], c=s["int_ior"], remap=False)


def parse_constant_emitter(rd):  # emitter.rs:43-65
    box = [(F(0),) * 3]

    def body(name, attrs, st):
        if name != "rgb":
            raise LoadError(f"Unknown constant emitter data type '{name}'")
        box[0] = parse_rgb(attrs, "radiance")

    parse_element(rd, body)
    return box[0]


def parse_point_light(rd):  # emitter.rs:67-115
    s = dict(p=[F(0), F(0), F(0)], I=(F(0),) * 3)

    def body(name, attrs, st):
        if name == "point":
            if find_attr(attrs, "name") != "position":
                raise LoadError("Expected 'name': 'filename' as first mesh 'string' attribute")
            for n, v in attrs[1:]:
                if n not in ("x", "y", "z"):
                    raise LoadError(f"Invalid point axis '{n}'")
                s["p"]["xyz".index(n)] = parse_f32(v, "point")
        elif name == "rgb":
            s["I"] = parse_rgb(attrs, "intensity")
        else:
            raise LoadError(f"Unknown light data type '{name}'")

    parse_element(rd, body)
    s["p"][0] = -s["p"][0]
    out = abi.LightDesc()
    binding.LightFactory.make_point_light(ol.translation(s["p"]).m, s["I"], out)
    return out


def parse_spot_light(rd):  # emitter.rs:117-163
    s = dict(xf=ol.Xf(), I=(F(0),) * 3, total=F(0), falloff=F(0))

    def body(name, attrs, st):
        if name == "float":
            n = find_attr(attrs, "name")
            if n == "cutoff_angle":
                s["total"] = parse_f32(find_attr(attrs, "value"), "float cutoff_angle")
            elif n == "beam_width":
                s["falloff"] = parse_f32(find_attr(attrs, "value"), "float beam_width")
            else:
                raise LoadError(f"Unexpected spot light float 'name': '{n}'")
        elif name == "transform":
            s["xf"] = parse_transform(rd)
            st.level -= 1
        elif name == "rgb":
            s["I"] = parse_rgb(attrs, "intensity")
        else:
            raise LoadError(f"Unknown spot light data type '{name}'")

    parse_element(rd, body)
    with np.errstate(all="ignore"):
        xf = ol.scale(-1.0, 1.0, 1.0) * s["xf"]
    out = abi.LightDesc()
    binding.LightFactory.make_spot_light(xf.m, xf.mi, s["I"], s["total"], s["falloff"], out)
    return out


def parse_shape(rd, dir_path, materials, shape_attrs, acc):  # shape.rs:19-94
    ty = find_attr(shape_attrs, "type")
    if ty != "ply":
        raise LoadError(f"Unexpected shape type '{ty}'!")
    s = dict(xf=ol.Xf(), path=None, mat=None)

    def body(name, attrs, st):
        if name == "string":
            if find_attr(attrs, "name") != "filename":
                raise LoadError("Expected 'name': 'filename' as mesh 'string' attribute")
            rel = find_attr(attrs, "value").replace("\\", "/")
            p = rel if rel.startswith("/") else dir_path + "/" + rel
            if not os.path.exists(p):
                raise LoadError(f"Could not open '{p}'")
            s["path"] = p
        elif name == "ref":
            rt = find_attr(attrs, "name")
            if rt != "bsdf":
                raise LoadError(f"Expected mesh 'ref' to be 'bsdf', got '{rt}'")
            s["mat"] = find_attr(attrs, "id")
        elif name == "transform":
            s["xf"] = parse_transform(rd)
            st.level -= 1
        else:
            raise LoadError(f"Unknown shape type '{name}'")

    parse_element(rd, body)
    with np.errstate(all="ignore"):
        xf = ol.scale(-1.0, 1.0, 1.0) * s["xf"]
    if s["path"] is None:
        raise LoadError("Mesh with no ply")
    if s["mat"] is None:
        raise LoadError("Mesh with no material")
    if s["mat"] not in materials:
        raise LoadError("Unknown mesh material '%s'" % s["mat"])
    try:
        ol._ply_mesh(acc, s["path"], xf, materials[s["mat"]])  # ply::load inside shape::parse: document order
    except (ValueError, KeyError, IndexError, OverflowError, MemoryError) as e:
        raise LoadError(f"PLY: {e}")
    except LoadError as e:
        raise LoadError(str(e) if "PLY" in str(e) else f"PLY: {e}")


def load_mitsuba(path, split_method=abi.SPLIT_SAH, max_shapes_in_node=1):
    """scene::mitsuba::load, mod.rs:28-218 -> (SceneData, CameraParameters, FilmSettings)."""
    path = os.fspath(path)
    if not os.path.isfile(path):
        raise LoadError(f"Could not open '{path}'")
    with open(path, "rb") as f:
        rd = _Reader(xml_events(f.read()))
    slash = path.rfind("/")
    dir_path = "." if slash < 0 else ("/" if slash == 0 else path[:slash])
    acc = ol._Accum()
    materials, lights = {}, []
    camera = dict(position=(F(0),) * 3, target=(F(0),) * 3, up=(F(0), F(1), F(0)), fov_axis=abi.FOV_X, fov_degrees=F(0))
    res = [640, 480]
    ignore = None
    while True:
        e = rd.next()
        if e[0] == "start":
            if ignore is None:
                name, attrs = e[1], e[2]
                if name == "scene":
                    if find_attr(attrs, "version") != "2.1.0":
                        raise LoadError("Scene file version is not 2.1.0")
                elif name == "default":
                    n, v = find_attr(attrs, "name"), find_attr(attrs, "value")
                    if n == "resx":
                        res[0] = parse_u16(v, "default resx")
                    elif n == "resy":
                        res[1] = parse_u16(v, "default resy")
                elif name == "integrator":
                    ignore = 0
                elif name == "sensor":
                    camera = parse_sensor(rd)
                elif name == "bsdf":
                    ty = find_attr(attrs, "type")
                    if ty == "twosided":
                        m = parse_twosided(rd)
                    elif ty == "diffuse":
                        m = parse_diffuse(rd)
                    elif ty == "dielectric":
                        m = parse_dielectric(rd)
                    else:
                        raise LoadError(f"Unknown bsdf type '{ty}'")
                    ident = find_attr(attrs, "id")
                    acc.materials.append(m)
                    materials[ident] = len(acc.materials) - 1
                elif name == "emitter":
                    ty = find_attr(attrs, "type")
                    if ty == "constant":
                        acc.background = parse_constant_emitter(rd)
                    elif ty == "point":
                        lights.append(parse_point_light(rd))
                    elif ty == "spot":
                        lights.append(parse_spot_light(rd))
                    else:
                        ignore = 0
                elif name == "shape":
                    parse_shape(rd, dir_path, materials, attrs, acc)
                else:
                    raise LoadError(f"Unknown element: '{name}'")
            if ignore is not None:
                ignore += 1
        elif e[0] == "end":
            if ignore is not None:
                after = ignore - 1
                ignore = after if after > 0 else None
        elif e[0] in ("error", "enddoc"):
            break
        else:
            _unexpected(e)
    if not acc.meshes:
        raise LoadError("mitsuba: scene has no shapes")
    sd = acc.finish(split_method, max_shapes_in_node, None, tuple(res), os.path.basename(path))
    sd.light_structs = lights
    # mod.rs:192-203: the target moves to the middle of the visible scene
    used = sd.points[sd.indices.ravel()]
    lo, hi = np.ascontiguousarray(used.min(axis=0), dtype=F), np.ascontiguousarray(used.max(axis=0), dtype=F)
    with np.errstate(all="ignore"):
        pos = np.array(camera["position"], dtype=F)
        fwd = ol.normalized(np.array(camera["target"], dtype=F) - pos)
        tmin, tmax = C.c_float(0), C.c_float(0)
        hit = binding.lib().orc_slab_test_f32(binding._p(lo), binding._p(hi), binding._p(pos), binding._p(np.ascontiguousarray(fwd, dtype=F)), float("inf"), C.byref(tmin), C.byref(tmax))
        if hit:
            p0, p1 = F(tmin.value), F(tmax.value)
            d = (p0 + p1) / F(2) if p0 > 0 else p1 / F(2)
            camera["target"] = tuple(pos + fwd * d)
    cam = dict(position=tuple(float(v) for v in camera["position"]), target=tuple(float(v) for v in camera["target"]), up=tuple(float(v) for v in camera["up"]),
               fov_axis=int(camera["fov_axis"]), fov_degrees=float(camera["fov_degrees"]))
    sd.camera = cam
    return sd, CameraParameters(**cam), FilmSettings(res=tuple(res), tile_dim=16)


# ------------------------------------------------------------------ comparison (the shape of tests/test_loaders.py's)
def _eq(a, b):
    if a is None or b is None:
        return a is b
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _f3(v):
    return np.array(v, dtype=F).tobytes()


def assert_same_loaded(want, got):
    """Every field of two (SceneData, CameraParameters, FilmSettings) triples, bit for bit."""
    (w, wc, wf), (g, gc, gf) = want, got
    for k in ("points", "normals", "uvs", "indices", "tri_mesh", "tri_material", "tri_area_light"):
        assert _eq(getattr(w, k), getattr(g, k)), k
    assert w.meshes == g.meshes
    assert len(w.materials) == len(g.materials)
    for a, b in zip(w.materials, g.materials):
        assert a["kind"] == b["kind"] and _f3(a["a"]) == _f3(b["a"]) and _f3(a["b"]) == _f3(b["b"]), (a, b)
        assert F(a["c"]).tobytes() == F(b["c"]).tobytes() and bool(a["remap"]) == bool(b["remap"]), (a, b)
    assert [bytes(x) for x in w.light_structs] == [bytes(x) for x in g.light_structs]
    assert _f3(w.background) == _f3(g.background)
    ident = np.arange(w.n_triangles, dtype=np.uint32)
    assert _eq(w.shape_order if w.shape_order is not None else ident, ident) and _eq(g.shape_order if g.shape_order is not None else ident, ident)
    assert not w.spheres and not g.spheres and not w.textures and not g.textures
    assert (w.split_method, w.max_shapes_in_node) == (g.split_method, g.max_shapes_in_node)
    assert _f3(wc.position) == _f3(gc.position), (wc.position, gc.position)
    assert _f3(wc.target) == _f3(gc.target), (wc.target, gc.target)
    assert _f3(wc.up) == _f3(gc.up), (wc.up, gc.up)
    assert wc.fov_axis == gc.fov_axis and F(wc.fov_degrees).tobytes() == F(gc.fov_degrees).tobytes()
    assert tuple(wf.res) == tuple(gf.res) and wf.tile_dim == gf.tile_dim == 16
