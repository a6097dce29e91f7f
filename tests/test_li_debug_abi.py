"""Integrator::li_debug and the ShadingUVs integrator at the C ABI, without a device: the ray record agrees between the
header, the ctypes mirror, the numpy dtype and the Rust declarations; the ray types keep the reference's order
(integrators/mod.rs:83-90); yk_li_debug fails loudly when there is no GPU."""
import ctypes as C
import os
import re

import numpy as np

from yuki_amd import _ffi, abi, core

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    return open(os.path.join(ROOT, "include", "yuki_hip.h")).read()


def test_integrator_ray_layout_agrees_everywhere():
    L = _ffi.lib()
    assert L.yk_sizeof(14) == 32 == C.sizeof(abi.IntegratorRay) == abi.INTEGRATOR_RAY_DTYPE.itemsize
    names = [f[0] for f in abi.IntegratorRay._fields_]
    assert names == ["o", "d", "t_max", "ray_type"] == list(abi.INTEGRATOR_RAY_DTYPE.names)
    for name in names:
        assert getattr(abi.IntegratorRay, name).offset == abi.INTEGRATOR_RAY_DTYPE.fields[name][1], name
    m = re.search(r"typedef struct yk_integrator_ray \{(.*?)\} yk_integrator_ray;", _header(), re.S)
    c_fields = [re.sub(r"\[.*?\]", "", d.strip().split()[-1]) for d in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(";") if d.strip()]
    assert c_fields == names
    rs = open(os.path.join(ROOT, "integration", "rust", "yuki_hip_sys", "src", "lib.rs")).read()
    rm = re.search(r"pub struct yk_integrator_ray \{(.*?)\n\}", rs, re.S)
    assert re.findall(r"pub (\w+):", rm.group(1)) == names
    assert "pub fn yk_li_debug(" in rs


def test_ray_types_follow_the_reference_order():
    want = ["DIRECT", "REFLECTION", "REFRACTION", "NORMAL", "SHADOW"]  # RayType, integrators/mod.rs:83-90
    hdr = _header()
    rs = open(os.path.join(ROOT, "integration", "rust", "yuki_hip_sys", "src", "lib.rs")).read()
    for k, name in enumerate(want):
        assert re.search(rf"YK_RAY_{name} = {k}\b", hdr), name
        assert re.search(rf"pub const YK_RAY_{name}: u32 = {k};", rs), name
        assert getattr(abi, f"RAY_{name}") == k
    assert [core.RayType.Direct, core.RayType.Reflection, core.RayType.Refraction, core.RayType.Normal, core.RayType.Shadow] == list(range(5))


def test_shading_uvs_is_kind_5():
    assert core.IntegratorType.ShadingUVs.kind == abi.INTEGRATOR_SHADING_UVS == 5
    assert re.search(r"YK_INTEGRATOR_SHADING_UVS = 5\b", _header())
    rs = open(os.path.join(ROOT, "integration", "rust", "yuki_hip_sys", "src", "lib.rs")).read()
    assert "pub const YK_INTEGRATOR_SHADING_UVS: u32 = 5;" in rs
    assert "static yk_integrator_desc ShadingUVs()" in open(os.path.join(ROOT, "include", "yuki_hip.hpp")).read()


def test_li_debug_without_a_device_fails_loudly():
    import torch

    if torch.cuda.is_available():
        return
    L = _ffi.lib()
    o = np.zeros((1, 3), dtype=np.float32)
    d = np.array([[0, 0, 1]], dtype=np.float32)
    pix = np.zeros((1, 2), dtype=np.uint16)
    si = np.zeros(1, dtype=np.uint32)
    li = np.zeros((1, 3), dtype=np.float32)
    cnt = np.zeros(1, dtype=np.uint32)
    recs = np.zeros(4, dtype=abi.INTEGRATOR_RAY_DTYPE)
    nr = np.zeros(1, dtype=np.uint32)
    smp = core.SamplerType.Uniform(1)
    integ = core.IntegratorType.Path(core.PathParams(max_depth=2))
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    st = L.yk_li_debug(None, None, C.byref(smp), C.byref(integ), 1, p(o), p(d), p(pix), p(si), 2, 4, p(li), p(cnt), p(recs), p(nr))
    assert st == 1  # YK_ERR_INVALID_ARGUMENT: no context
    h = C.c_void_p()
    assert L.yk_context_create(0, C.byref(h)) == 2 and not h.value  # YK_ERR_NO_DEVICE: nothing to call it on, no CPU path
