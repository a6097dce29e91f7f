"""yk_scene_create_device / Scene.from_device without a GPU: the symbol is exported and bound, a NULL context is
refused, and the Python entry point checks its tensors before it calls the library."""
import ctypes as C
import types

import numpy as np
import pytest

from yuki_amd import _ffi, abi, scenes

try:
    import torch
except ImportError:  # the two ABI tests run without it
    torch = None
needs_torch = pytest.mark.skipif(torch is None, reason="Scene.from_device checks torch tensors")


def test_the_symbol_is_exported_and_bound(yk):
    assert "yk_scene_create_device" in _ffi.SYMBOLS
    f = yk.lib().yk_scene_create_device
    assert f.restype is C.c_int and len(f.argtypes) == 4


def test_a_null_context_is_refused(yk):
    d, keep = scenes.by_name("city-tiny").desc(yk.LightFactory)
    h = C.c_void_p()
    assert yk.lib().yk_scene_create_device(None, C.byref(d), None, C.byref(h)) == 1  # YK_ERR_INVALID_ARGUMENT
    assert not h.value
    del keep


class _NoLibrary:
    """Stands in for the loaded library: any call through it fails the test."""

    def __getattr__(self, name):
        raise AssertionError(f"{name} was called before the tensors were checked")


@pytest.fixture()
def checked_only(yk, monkeypatch):
    monkeypatch.setattr(yk, "lib", lambda: _NoLibrary())
    return types.SimpleNamespace(device=0, h=None)  # a context is not needed to refuse a tensor


def _tensors(sd):
    return dict(points=torch.from_numpy(np.ascontiguousarray(sd.points, dtype=np.float32)), indices=torch.from_numpy(np.ascontiguousarray(sd.indices, dtype=np.uint32).view(np.int32)),
                tri_material=torch.from_numpy(np.ascontiguousarray(sd.tri_material, dtype=np.int32)))


@needs_torch
def test_a_wrong_element_type_is_refused(yk, checked_only):
    sd = scenes.by_name("city-tiny")
    for name, wrong in (("points", torch.float64), ("indices", torch.int64), ("tri_material", torch.float32)):
        t = _tensors(sd)
        t[name] = t[name].to(wrong)
        with pytest.raises(ValueError, match=name):
            yk.Scene.from_device(checked_only, sd, t)


@needs_torch
def test_a_tensor_that_is_not_contiguous_is_refused(yk, checked_only):
    sd = scenes.by_name("city-tiny")
    t = _tensors(sd)
    t["points"] = torch.zeros((3, len(sd.points)), dtype=torch.float32).t()  # the right shape, the wrong strides
    assert t["points"].shape == (len(sd.points), 3) and not t["points"].is_contiguous()
    with pytest.raises(ValueError, match="points.*contiguous"):
        yk.Scene.from_device(checked_only, sd, t)


@needs_torch
def test_a_short_tensor_is_refused(yk, checked_only):
    sd = scenes.by_name("city-tiny")
    for name in ("points", "indices", "tri_material"):
        t = _tensors(sd)
        t[name] = t[name][:-1].contiguous()
        with pytest.raises(ValueError, match=f"{name}.*elements"):
            yk.Scene.from_device(checked_only, sd, t)
    t = _tensors(sd)
    t["shape_order"] = torch.arange(sd.n_triangles - 1, dtype=torch.int32)
    with pytest.raises(ValueError, match="shape_order.*elements"):
        yk.Scene.from_device(checked_only, sd, t)


@needs_torch
def test_host_tensors_and_unknown_names_are_refused(yk, checked_only):
    sd = scenes.by_name("city-tiny")
    with pytest.raises(ValueError, match="not on the context's device"):
        yk.Scene.from_device(checked_only, sd, _tensors(sd))
    with pytest.raises(ValueError, match="unknown device arrays"):
        yk.Scene.from_device(checked_only, sd, dict(_tensors(sd), vertices=0))
    assert set(yk.Scene.DEVICE_ARRAYS) == {f for f, _ in abi.SceneDesc._fields_ if f in ("points", "normals", "uvs", "indices", "tri_mesh", "tri_material", "tri_area_light", "shape_order")}


@needs_torch
def test_scene_update_refuses_tensors_with_the_messages_of_from_device(yk, checked_only):
    """Scene.update and Scene.from_device check their tensors with one helper: wrong element type, wrong strides, a short
    tensor and a host tensor raise the same text from both, before the library is reached."""
    sd = scenes.by_name("city-tiny")
    nv = len(sd.points)
    scene = yk.Scene.__new__(yk.Scene)
    scene.ctx, scene.data, scene.h = checked_only, sd, None
    good = _tensors(sd)["points"]
    bad = {"element type": good.to(torch.float64), "contiguous": torch.zeros((3, nv), dtype=torch.float32).t(), "elements": good[:-1].contiguous(), "not on the context's device": good}
    for what, points in bad.items():
        with pytest.raises(ValueError, match=what) as from_update:
            scene.update(points)
        with pytest.raises(ValueError, match=what) as from_create:
            yk.Scene.from_device(checked_only, sd, dict(_tensors(sd), points=points))
        assert str(from_update.value) == str(from_create.value) and str(from_update.value).startswith("points: ")
    with pytest.raises(ValueError, match="normals: .*float64"):  # every array's shape and type before any array's place
        scene.update(good, good.to(torch.float64))
