#!/usr/bin/env python3
"""Scene creation from host arrays against scene creation from tensors already on the device, one process.

For each scene (default cfg3 and cfg5, SAH, one shape per leaf), after one warm-up of each, the two alternate,
`--runs` calls each, and the wall time of the whole call is taken (host clock around it; both end synchronised):

  host input    yk_scene_create with "bvh_builder" = 1 and "scene_layout" = 1, from numpy arrays
  device input  yk_scene_create_device (Scene.from_device) from torch tensors that are resident before the clock starts

The warm-up compares the seven device record buffers of the two (bytes) and checks that neither fell back.  Reported per
scene: every run, the fastest host-input run and the slowest device-input run.

    python tools/scene_input_bench.py --out profiles/scene_from_device.json
"""
import argparse
import hashlib
import json
import os
import sys
import time

import numpy as np
import torch  # before the library: one process holds one HIP runtime (tests/conftest.py)

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from yuki_amd import abi, scenes  # noqa: E402
from yuki_amd import core as yk  # noqa: E402

UNSIGNED = ("indices", "tri_mesh", "shape_order")


def tensors(sd):
    out = {}
    for name, dtype in (("points", np.float32), ("normals", np.float32), ("uvs", np.float32), ("indices", np.uint32), ("tri_mesh", np.uint32), ("tri_material", np.int32), ("tri_area_light", np.int32),
                        ("shape_order", np.uint32)):
        a = getattr(sd, name)
        if a is not None:
            a = np.ascontiguousarray(a, dtype=dtype)
            out[name] = torch.from_numpy(a.view(np.int32) if name in UNSIGNED else a).to("cuda:0")
    torch.cuda.synchronize()
    return out


def create(make):
    t0 = time.perf_counter()
    s = make()
    wall = time.perf_counter() - t0
    i, bi, li = s.info(), s.build_info(), s.layout_info()
    assert (bi.builder, bi.reason, li.layout, li.reason) == (1, 0, abi.LAYOUT_DEVICE, 0), (bi.builder, bi.reason, li.layout, li.reason)
    return s, dict(scene_create_seconds=wall, build_seconds=i.build_seconds, upload_seconds=i.upload_seconds, builder_seconds_upload=bi.seconds_upload, layout_seconds_upload=li.seconds_upload,
                   layout_seconds_layout=li.seconds_layout, n_nodes=int(i.n_nodes), device_bytes=int(i.device_bytes))


def digest(s):
    return [hashlib.sha256(s.device_records(name).tobytes()).hexdigest() for name in abi.RECORD_NAMES]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="cfg3,cfg5")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    host_ctx, dev_ctx = yk.Context(0, bvh_builder=1, scene_layout=1), yk.Context(0)
    result = dict(tool="tools/scene_input_bench.py", split_method="SAH", max_shapes_in_node=1, scenes={})
    for name in a.scenes.split(","):
        sd = scenes.by_name(name)
        sd.split_method, sd.max_shapes_in_node = abi.SPLIT_SAH, 1
        resident = tensors(sd)
        makers = dict(host_input=lambda: yk.Scene(host_ctx, sd), device_input=lambda: yk.Scene.from_device(dev_ctx, sd, resident))
        out = dict(n_shapes=int(sd.n_triangles), geometry_bytes=int(sum(t.numel() * t.element_size() for t in resident.values())), host_input=[], device_input=[])
        want = None
        for which, make in makers.items():  # warm-up, and the comparison
            s, _ = create(make)
            got = digest(s)
            assert want is None or got == want, "the device-input scene's records differ from the host-input scene's"
            want = got
            s.close()
        for k in range(a.runs):
            for which, make in makers.items():
                s, rec = create(make)
                s.close()
                out[which].append(rec)
                print(f"{name} {which} #{k}: scene_create {rec['scene_create_seconds']:.4f} s (build {rec['build_seconds']:.4f}, upload {rec['upload_seconds']:.4f})", flush=True)
        out["host_input_fastest_seconds"] = min(r["scene_create_seconds"] for r in out["host_input"])
        out["device_input_slowest_seconds"] = max(r["scene_create_seconds"] for r in out["device_input"])
        out["device_input_fastest_seconds"] = min(r["scene_create_seconds"] for r in out["device_input"])
        out["device_slowest_over_host_fastest"] = out["device_input_slowest_seconds"] / out["host_input_fastest_seconds"]
        result["scenes"][name] = out
        del resident
        torch.cuda.empty_cache()
    print(json.dumps(result))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
