#!/usr/bin/env python3
"""What the tests compare with the reference's text, reduced to numbers and names: tests/golden/reference_facts.json.

The reference (a Rust crate) is not part of this repository.  This script reads a checkout of it as text and stores only
data — cfg1's scene constants, the pbrt loader's parameter defaults, the copper tables and CIE fit constants, the loop of
`permutation_element`, the float literals of the files on the render path, and the names and line ranges of the reference's
own unit tests — so that tests/test_reference_constants.py and tests/test_oracle_math.py run without it.

    python tools/reference_facts.py REFERENCE_DIR      # rewrites tests/golden/reference_facts.json
"""
import json
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import reference_cornell_check as rc  # noqa: E402

OUT = rc.FACTS
PBRT_RS = "yuki/src/scene/pbrt/mod.rs"
CIE_RS = "yuki/src/scene/pbrt/cie.rs"
STRATIFIED_RS = "yuki/src/sampling/stratified.rs"
SRC = "yuki/src/"
UNIT_TESTS = "tests/src"
UNIT_TEST_FILES = ["transform", "matrix", "vector", "bounds", "point", "normal", "ray"]
# the reference files on the render path whose float literals must appear in the oracle and in the product
PATH_FILES = ["materials/bsdfs/trowbridge_reitz.rs", "materials/bsdfs/oren_nayar.rs", "materials/bsdfs/fresnel.rs", "materials/bsdfs/microfacet.rs",
              "materials/bsdfs/specular.rs", "materials/bsdfs/lambertian.rs", "materials/bsdfs/mod.rs", "sampling/mod.rs", "integrators/path.rs",
              "integrators/whitted.rs", "interaction.rs", "visibility.rs", "shapes/triangle.rs", "shapes/sphere.rs", "lights/point_light.rs",
              "lights/spot_light.rs", "lights/distant_light.rs", "lights/rectangular_light.rs", "camera.rs", "bvh.rs", "math/bounds.rs"]


def load():
    with open(OUT) as f:
        return json.load(f)


def float_literals(text):
    """Every floating-point literal of a Rust or C++ text outside comments, as the set of binary32 values."""
    text = re.sub(r"//[^\n]*", "", text)
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    out = set()
    for m in re.finditer(r"(?<![\w.])(\d[\d_]*\.[\d_]*(?:e-?\d+)?|\d[\d_]*e-?\d+)(?:_?f32|f)?(?![\w.])", text):
        out.add(float(np.float32(float(m.group(1).replace("_", "")))))
    return out


def rust_f32_array(src, name):
    body = re.search(r"const %s: \[f32; \w+\] = \[(.*?)\];" % name, src, re.S).group(1)
    return [float(np.float32(float(v.replace("_", "")))) for v in re.findall(r"-?\d[\d_]*\.?[\d_]*(?:e-?\d+)?", body)]


def permutation_steps(text, start, stop):
    """The loop body between `start` and `stop` as a normalised sequence of (operator, constant-or-shift) steps."""
    body = text[text.index(start):]
    body = body[:body.index(stop)]
    out = []
    for line in body.splitlines():
        line = line.strip().rstrip(";")
        m = re.match(r"i = i\.wrapping_mul\((.*)\)$", line) or re.match(r"i \*= (.*)$", line)
        if m:
            out.append(["mul", m.group(1).replace("u", "").replace(" ", "").lower()])
            continue
        m = re.match(r"i \^= (.*)$", line)
        if m:
            out.append(["xor", m.group(1).replace(" ", "")])
            continue
        m = re.match(r"i &= (.*)$", line)
        if m:
            out.append(["and", m.group(1).replace(" ", "")])
    return out


def pbrt_defaults(src):
    """Every `params.find_*("name", default)` of scene/pbrt/mod.rs in order of appearance, the default evaluated."""
    src = re.sub(r"\s+", " ", src)
    variables = {}
    for name, value in (("default_l", "Spectrum::ones()"), ("default_i", "Spectrum::ones()"), ("default_pos", "Point3::zeros()")):
        assert f"let {name} = {value};" in src, name
        variables[name] = value
    triple = lambda t: [float(v) for v in re.fullmatch(r"\w+::new\(([-\d.]+), ([-\d.]+), ([-\d.]+)\)", t).groups()]

    def value(kind, text):
        text = variables.get(text, text)
        if kind in ("f32", "i32"):
            return float(text)
        if kind == "bool":
            return {"true": True, "false": False}[text]
        if kind == "string":
            return json.loads(text)
        if text in ("Spectrum::ones()", "Point3::ones()"):
            return [1.0, 1.0, 1.0]
        if text in ("Spectrum::zeros()", "Point3::zeros()"):
            return [0.0, 0.0, 0.0]
        m = re.fullmatch(r"sampled_spectrum_into_rgb\(&COPPER_WAVELENGTHS, &COPPER_(N|K)\)", text)
        if m:
            return {"copper": m.group(1).lower()}
        return triple(text)

    out = []
    for m in re.finditer(r'find_(f32|i32|bool|spectrum|point|string)\( ?"(\w+)", ?', src):
        depth, j = 1, m.end()
        while depth:  # the default runs to the call's closing parenthesis
            depth += {"(": 1, ")": -1}.get(src[j], 0)
            j += 1
        out.append(dict(type=m.group(1), name=m.group(2), default=value(m.group(1), src[m.end():j - 1].strip().rstrip(",").strip())))
    return out


def unit_tests(path):
    """(name, first line, last line) of every `#[test]` function of one file."""
    lines = open(path).read().split("\n")
    out = []
    i = 0
    while i < len(lines):
        if lines[i].strip() == "#[test]":
            j = i + 1
            m = re.search(r"fn\s+([a-z_0-9]+)", lines[j])
            depth, k, seen = 0, j, False
            while k < len(lines):
                depth += lines[k].count("{") - lines[k].count("}")
                seen = seen or "{" in lines[k]
                if seen and depth == 0:
                    break
                k += 1
            out.append([m.group(1), j + 1, k + 1])
            i = k
        i += 1
    return out


def extract(ref_dir):
    read = lambda rel: open(os.path.join(ref_dir, rel)).read()
    pbrt = read(PBRT_RS)
    cie = read(CIE_RS)
    cie = cie[cie.index("pub fn x_fit_1931"):]
    return dict(
        cornell=rc.parse_reference(ref_dir),
        pbrt_defaults=pbrt_defaults(pbrt),
        copper={key: rust_f32_array(pbrt, name) for name, key in (("COPPER_WAVELENGTHS", "wavelengths"), ("COPPER_N", "n"), ("COPPER_K", "k"))},
        # every float literal of cie.rs's fits, in order; the XYZ -> RGB matrix of pbrt/mod.rs, in order (absolute values)
        cie_fit_literals=[float(np.float32(v)) for v in re.findall(r"(?<![\w.])\d+\.\d+", cie)],
        xyz_to_rgb=[float(np.float32(v.replace("_", ""))) for v in re.findall(r"(?<![\w.])\d\.[\d_]+", pbrt[pbrt.index("3.240_479"):pbrt.index("fn is_sorted")])],
        permutation_element=permutation_steps(read(STRATIFIED_RS), "loop {", "if i < l"),
        path_literals={f: sorted(float_literals(read(SRC + f))) for f in PATH_FILES},
        unit_tests={f: unit_tests(os.path.join(ref_dir, UNIT_TESTS, f + ".rs")) for f in UNIT_TEST_FILES},
    )


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    facts = extract(sys.argv[1])
    with open(OUT, "w") as f:
        json.dump(facts, f, indent=1)
        f.write("\n")
    print(f"-> {os.path.relpath(OUT, ROOT)}")


if __name__ == "__main__":
    main()
