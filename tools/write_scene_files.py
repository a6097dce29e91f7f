#!/usr/bin/env python3
"""BASELINE.json's configurations as the FILES its text names ("Stanford-bunny PLY", "~1 M-tri pbrt-v3 scene"): the generated
meshes of yuki_amd/scenes.py written in the formats the reference's loaders read (tests/scene_files.py), for
`bench.py --scene-file` and the loader tests.

    python tools/write_scene_files.py cfg2 out_dir     ->  out_dir/bunny_class.ply
    python tools/write_scene_files.py cfg3 out_dir     ->  out_dir/scene.pbrt + out_dir/meshes/m*.ply (802 files)
    python tools/write_scene_files.py cfg5 out_dir     ->  the 10,240,012-triangle city (8002 PLY files, 0.4 GB)
    python tools/write_scene_files.py --format mitsuba cfg3 out_dir   ->  out_dir/scene.xml + out_dir/meshes/m*.ply
                                                        (Mitsuba 2.1.0, tests/mitsuba_files.py: x negated on the way out, the
                                                        loader mirrors it back, faces with reversed winding so that the
                                                        mirrored meshes are not inside out; glass -> dielectric, the rest -> diffuse)

The pbrt variant of a city has no rectangular area light (the reference's pbrt loader parses AreaLightSource and ignores it,
scene/pbrt/mod.rs:502): its quad stays as black geometry, the two point lights and the background remain."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import mitsuba_files as mf  # noqa: E402
import scene_files as sf  # noqa: E402

from yuki_amd import scenes  # noqa: E402


def main():
    args = sys.argv[1:]
    fmt = "native"
    if args and args[0] == "--format":
        fmt, args = args[1], args[2:]
    name, out = args[0], args[1]
    os.makedirs(out, exist_ok=True)
    t0 = time.time()
    if fmt == "mitsuba":
        res = (3840, 2160) if name == "cfg5" else (1920, 1080)
        p, _, info = mf.write_scene_as_mitsuba(scenes.by_name(name), out, res=res, twosided=name == "cfg2", reverse_winding=True)
        print(info, file=sys.stderr)
    elif fmt != "native":
        sys.exit("unknown --format '%s' (native, mitsuba)" % fmt)
    elif name == "cfg2":
        p = sf.write_cfg2_ply(os.path.join(out, "bunny_class.ply"))
    else:
        res = (3840, 2160) if name == "cfg5" else (1920, 1080)
        p, info = sf.write_scene_as_pbrt(out, scenes.by_name(name), res=res)
        print(info, file=sys.stderr)
    print(f"{p}  ({time.time() - t0:.1f} s)", file=sys.stderr)
    print(p)


if __name__ == "__main__":
    main()
