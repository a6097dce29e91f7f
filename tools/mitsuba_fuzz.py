#!/usr/bin/env python3
"""Seeded random Mitsuba 2.1.0 files for the loader comparison (tests/test_mitsuba_fuzz.py): a valid file built from random
choices, then mutated — attributes and children dropped, duplicated and reordered, numbers respelled (`1.`, `.5`, `1e-3`,
`+2`, `inf`, doubled spaces), ignored subtrees nested, elements renamed, and the three kinds of malformed XML the loader
keeps the reference's behaviour for (the file ends inside an element, an end tag that does not match, a repeated
attribute).  Not generated: zero rotation axes, non-finite numbers where they would reach arithmetic (the sign of a NaN is
the platform's), other malformed XML.

    python tools/mitsuba_fuzz.py OUT_DIR SEED [SEED ...]    # writes OUT_DIR/fuzz_SEED.xml beside the PLY files they name
    python tools/mitsuba_fuzz.py --rate N                   # how many of seeds 0..N-1 the checker alone accepts
"""
import copy
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

PLY_FILES = ["cube.ply", "geo/cube_le.ply", "geo/cube_be.ply", "geo/cube_n.ply", "geo\\cube_be.ply"]


def E(tag, attrs=(), children=(), keep=False):
    return dict(tag=tag, attrs=[list(a) for a in attrs], children=list(children), keep=keep)


def spell(rng, v):
    """One of the spellings str::parse::<f32> accepts for v."""
    if v == int(v) and abs(v) < 1000:
        i = int(v)
        return rng.choice(["%d" % i, "%d." % i, "%d.0" % i, "%de0" % i, ("+%d" % i) if i >= 0 else "%d" % i, "%.1fE+0" % v])
    s = "%.6g" % v
    if abs(v) < 1 and rng.random() < 0.4:
        s = s.replace("0.", ".", 1)
    if rng.random() < 0.2:
        s = "%.5e" % v
    return s


def nums(rng, n, lo, hi):
    return " ".join(spell(rng, rng.choice([round(rng.uniform(lo, hi), rng.randint(0, 3)), float(rng.randint(int(lo), int(hi)))])) for _ in range(n))


def nonzero(rng):
    return rng.choice([-1, 1]) * round(rng.uniform(0.2, 1.0), 2)


def transform(rng, camera=False):
    kids = []
    for _ in range(rng.randint(0, 4)):
        k = rng.choice(["rotate", "translate", "scale", "matrix"] if not camera else ["rotate", "translate", "rotate"])
        if k == "rotate":
            kids.append(E("rotate", [("x", spell(rng, nonzero(rng))), ("y", spell(rng, nonzero(rng))), ("z", spell(rng, nonzero(rng))), ("angle", spell(rng, round(rng.uniform(-180, 180), 1)))]))
        elif k == "translate":
            kids.append(E("translate", [("value", nums(rng, 3, -4, 4))]))
        elif k == "scale":
            kids.append(E("scale", [("value", " ".join(spell(rng, rng.choice([0.5, 1.5, 2.0, -1.0, 0.25, 3.0])) for _ in range(rng.choice([1, 3]))))]))
        else:
            m = [rng.choice([-2.0, -1.0, -0.5, 0.5, 1.0, 2.0]) if r == c else round(rng.uniform(-0.3, 0.3), 2) for r in range(3) for c in range(4)]
            kids.append(E("matrix", [("value", " ".join(spell(rng, v) for v in m + [0.0, 0.0, 0.0, 1.0]))]))
    return E("transform", [("name", "to_world")], kids)


def ignored_subtree(rng, depth=0):
    kids = [ignored_subtree(rng, depth + 1) for _ in range(rng.randint(0, 2 if depth < 2 else 0))]
    tag = rng.choice(["integer", "float", "emitter", "shape", "bsdf", "sampler", "string", "scene"])
    return E(tag, [("name", "n%d" % rng.randint(0, 9)), ("value", spell(rng, rng.randint(0, 64)))], kids)


def rgb(rng, name, n=3):
    return E("rgb", [("name", name), ("value", nums(rng, n, 0, 1))])


def bsdf(rng, ident):
    k = rng.choice(["diffuse", "diffuse", "twosided", "dielectric"])
    if k == "diffuse":
        return E("bsdf", [("type", k), ("id", ident)], [rgb(rng, "reflectance", rng.choice([1, 2, 3, 3]))] if rng.random() < 0.8 else [])
    if k == "twosided":
        inner = rng.choice([[], [rgb(rng, "reflectance")], [E("bsdf", [("type", rng.choice(["diffuse", "plastic"]))], [rgb(rng, "reflectance")])]])
        return E("bsdf", [("type", k), ("id", ident)], inner)
    kids = []
    if rng.random() < 0.6:
        kids.append(E("float", [("name", "int_ior"), ("value", spell(rng, round(rng.uniform(1.1, 2.4), 3)))]))
    if rng.random() < 0.4:
        kids.append(E("float", [("name", "ext_ior"), ("value", rng.choice(["1.000277", "1.0003", "1", "1.001", "1.0015", "1.33"]))]))
    if rng.random() < 0.5:
        kids.append(rgb(rng, "specular_reflectance"))
    if rng.random() < 0.5:
        kids.append(rgb(rng, "specular_transmittance"))
    rng.shuffle(kids)
    return E("bsdf", [("type", k), ("id", ident)], kids)


def emitter(rng):
    k = rng.choice(["constant", "point", "spot", "area"])
    if k == "constant":
        return E("emitter", [("type", k)], [rgb(rng, "radiance")])
    if k == "point":
        axes = [(a, spell(rng, round(rng.uniform(-5, 5), 2))) for a in rng.sample("xyz", rng.randint(1, 3))]
        return E("emitter", [("type", k)], [dict(E("point", [("name", "position")] + axes), ordered=True), rgb(rng, "intensity")])
    if k == "spot":
        kids = [E("float", [("name", "cutoff_angle"), ("value", spell(rng, rng.randint(20, 60)))]), E("float", [("name", "beam_width"), ("value", spell(rng, rng.randint(5, 20)))]),
                transform(rng), rgb(rng, "intensity")]
        rng.shuffle(kids)
        return E("emitter", [("type", k)], kids)
    return E("emitter", [("type", k)], [ignored_subtree(rng) for _ in range(rng.randint(0, 2))])


def shape(rng, ids):
    kids = [E("string", [("name", "filename"), ("value", rng.choice(PLY_FILES))]), E("ref", [("name", "bsdf"), ("id", rng.choice(ids))])]
    if rng.random() < 0.8:
        kids.append(transform(rng))
    rng.shuffle(kids)
    return E("shape", [("type", "ply")], kids)


def base_scene(rng):
    top = [E("default", [("name", rng.choice(["resx", "resy", "spp"])), ("value", "%d" % rng.randint(1, 4000))]) for _ in range(rng.randint(0, 3))]
    if rng.random() < 0.5:
        top.append(E("integrator", [("type", "path")], [ignored_subtree(rng) for _ in range(rng.randint(0, 2))]))
    sensor_kids = [E("string", [("name", "fov_axis"), ("value", rng.choice("xy"))]), E("float", [("name", "fov"), ("value", spell(rng, round(rng.uniform(20, 90), 1)))]), transform(rng, camera=True)]
    if rng.random() < 0.5:
        sensor_kids.append(E("float", [("name", rng.choice(["near_clip", "far_clip"])), ("value", rng.choice(["0.01", "1e3", "inf", "1e-2"]))]))
    if rng.random() < 0.6:
        sensor_kids.append(E(rng.choice(["sampler", "film"]), [("type", "x")], [ignored_subtree(rng) for _ in range(rng.randint(0, 2))]))
    rng.shuffle(sensor_kids)
    top.append(E("sensor", [("type", "perspective")], sensor_kids, keep=True))
    ids = ["m%d" % k for k in range(rng.randint(1, 3))]
    mats = [bsdf(rng, i) for i in ids]
    if rng.random() < 0.3:
        mats.append(bsdf(rng, ids[0]))  # a material id defined twice
    lights = [emitter(rng) for _ in range(rng.randint(0, 3))]
    shapes = [shape(rng, ids) for _ in range(rng.randint(1, 3))]
    body = mats + lights
    rng.shuffle(body)
    if rng.random() < 0.3 and len(shapes) > 1:  # material and emitter elements between shapes
        body.insert(rng.randint(0, len(body)), shapes.pop(0))
    return E("scene", [("version", "2.1.0")], top + body + shapes, keep=True)


def walk(node, out=None, parent=None):
    out = [] if out is None else out
    out.append((node, parent))
    for c in node["children"]:
        walk(c, out, node)
    return out


RENAMES = ["bsdf", "shape", "emitter", "rgb", "float", "transform", "translate", "texture", "sensor", "integrator", "medium", "spectrum", "string", "ref"]
RESPELL = ["1.", ".5", "1e-3", "+2", "2.5E1", "007"]


def mutate(rng, root):
    """One structural mutation in place; returns its name."""
    nodes = walk(root)
    kind = rng.choice(["drop_attr", "dup_attr", "reorder_point", "drop_child", "dup_child", "reorder_children", "respell", "double_space", "inf", "nest_ignored", "rename"])
    if kind == "drop_attr":
        cand = [n for n, _ in nodes if n["attrs"]]
        n = rng.choice(cand)
        del n["attrs"][rng.randrange(len(n["attrs"]))]
    elif kind == "dup_attr":
        n = rng.choice([n for n, _ in nodes if n["attrs"]])
        a = rng.choice(n["attrs"])
        n["attrs"].insert(rng.randint(0, len(n["attrs"])), [a[0], a[1] if rng.random() < 0.5 else "1"])
    elif kind == "reorder_point":
        cand = [n for n, _ in nodes if n["tag"] == "point"]
        if cand:
            rng.shuffle(rng.choice(cand)["attrs"])
    elif kind == "drop_child":
        cand = [(n, c) for n, _ in nodes for c in n["children"] if not c["keep"]]
        if cand:
            n, c = rng.choice(cand)
            n["children"].remove(c)
    elif kind == "dup_child":
        cand = [(n, c) for n, _ in nodes for c in n["children"]]
        n, c = rng.choice(cand)
        n["children"].insert(rng.randint(0, len(n["children"])), copy.deepcopy(c))
    elif kind == "reorder_children":
        n = rng.choice([n for n, _ in nodes if len(n["children"]) > 1])
        rng.shuffle(n["children"])
    elif kind in ("respell", "double_space", "inf"):
        ok = {"respell": ("rgb", "translate", "scale", "float", "point"), "double_space": ("rgb", "translate", "scale", "matrix"), "inf": ("rgb",)}[kind]
        cand = [(n, a) for n, p in nodes for a in n["attrs"] if n["tag"] in ok and a[0] in ("value", "x", "y", "z") and not (n["tag"] == "float" and dict(map(tuple, n["attrs"])).get("name") == "ext_ior")]
        if cand:
            n, a = rng.choice(cand)
            parts = a[1].split(" ")
            k = rng.randrange(len(parts))
            if kind == "respell":
                parts[k] = rng.choice(RESPELL)
            elif kind == "inf":
                parts[k] = rng.choice(["inf", "Infinity", "+INF"])
            else:
                parts[k] = parts[k] + " "
            a[1] = " ".join(parts)
    elif kind == "nest_ignored":
        n = rng.choice([n for n, _ in nodes if n["tag"] in ("scene", "sensor", "integrator")])
        tag = "integrator" if n["tag"] == "scene" else rng.choice(["sampler", "film"]) if n["tag"] == "sensor" else "integer"
        sub = E(tag, [("type", "x")], [ignored_subtree(rng) for _ in range(rng.randint(1, 3))]) if n["tag"] != "scene" or rng.random() < 0.5 else E("emitter", [("type", "sky")], [ignored_subtree(rng), shape(rng, ["nope"])])
        n["children"].insert(rng.randint(0, len(n["children"])), sub)
    else:
        cand = [n for n, p in nodes if p is not None]
        rng.choice(cand)["tag"] = rng.choice(RENAMES)
    return kind


def serialize(rng, node, depth=0):
    """The tree as text, with random but harmless layout: either quote, white space inside tags, comments, both forms of an
    empty element; attribute order is shuffled except where the loader depends on it (<point>)."""
    attrs = list(node["attrs"])
    if not node.get("ordered") and rng.random() < 0.3:
        rng.shuffle(attrs)
    q = lambda v: ('"%s"' % v) if rng.random() < 0.8 or "'" in v else ("'%s'" % v)  # noqa: E731
    head = node["tag"] + "".join(rng.choice([" ", "  ", "\n" + "  " * (depth + 2)]) + "%s%s=%s%s" % (a[0], rng.choice(["", "", " "]), rng.choice(["", "", " "]), q(a[1])) for a in attrs)
    pad = "  " * depth
    if not node["children"]:
        return pad + (("<%s/>" % head) if rng.random() < 0.7 else ("<%s%s></%s%s>" % (head, rng.choice(["", " "]), node["tag"], rng.choice(["", " "])))) + "\n"
    out = pad + "<%s>\n" % head
    for c in node["children"]:
        if rng.random() < 0.1:
            out += pad + "  <!-- %s -->\n" % rng.choice(["note", "a < b & c", "<shape type='obj'/>"])
        out += serialize(rng, c, depth + 1)
    return out + pad + "</%s>\n" % node["tag"]


def generate(seed):
    """-> (text, [mutation names])"""
    rng = random.Random(0x4D495453 ^ (seed * 0x9E3779B1))
    root = base_scene(rng)
    done = [mutate(rng, root) for _ in range(rng.choice([0, 0, 0, 0, 1, 1, 1, 2, 2, 3]))]
    text = rng.choice(['<?xml version="1.0" encoding="utf-8"?>\n', "<?xml version='1.0'?>\n", "", "\n"]) + serialize(rng, root)
    r = rng.random()
    if r < 0.05:  # the file ends inside an element
        text = text[: rng.randint(len(text) // 3, len(text) - 1)]
        done.append("truncate")
    elif r < 0.09 and "</" in text:  # an end tag that does not match
        ends = [i for i in range(len(text)) if text.startswith("</", i)]
        i = rng.choice(ends)
        text = text[: i + 2] + "x" + text[i + 2 :]
        done.append("end_tag")
    return text, done


def write_case(dirname, seed):
    import mitsuba_files as mf

    if not os.path.exists(os.path.join(dirname, "geo", "cube_n.ply")):
        mf.write_hand_plys(dirname)
    text, done = generate(seed)
    p = os.path.join(dirname, "fuzz_%d.xml" % seed)
    with open(p, "w", encoding="utf-8") as f:
        f.write(text)
    return p, done


def main():
    if sys.argv[1] == "--rate":
        import tempfile

        import mitsuba_ref as mr

        n, ok, kinds = int(sys.argv[2]), 0, {}
        with tempfile.TemporaryDirectory() as d:
            for seed in range(n):
                p, done = write_case(d, seed)
                try:
                    mr.load_mitsuba(p)
                    ok += 1
                    good = True
                except mr.LoadError:
                    good = False
                for k in done or ["none"]:
                    a = kinds.setdefault(k, [0, 0])
                    a[0] += good
                    a[1] += 1
        print("accepted by the checker: %d of %d" % (ok, n))
        for k, (a, b) in sorted(kinds.items()):
            print("  %-18s %3d / %3d" % (k, a, b))
        return
    out = sys.argv[1]
    os.makedirs(out, exist_ok=True)
    for s in sys.argv[2:]:
        print(write_case(out, int(s))[0])


if __name__ == "__main__":
    main()
