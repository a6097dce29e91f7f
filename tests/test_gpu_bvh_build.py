"""The device BVH builder ("bvh_builder" = 1, yuki_amd/csrc/yk_bvh_build.hip) builds the host recursion's tree:
the same 32-byte nodes in the same depth-first order, the same shape order, counts and depth — on every scene
named here the device path is taken (no fallback), and what is rendered through a device-built scene is what is
rendered through a host-built one, bit for bit."""
import numpy as np
import pytest

from yuki_amd import abi, scenes

from test_bvh_levels import SCENES, TABLE, _one_and_seven, _signed_zero_scene, _tree
from test_scene_layout_plan import _seam_scene

pytestmark = pytest.mark.gpu
SEED = 0x73B9642E74AC471C
HOST, DEVICE = 0, 1
REASON_SPLIT_METHOD = 1


@pytest.fixture(scope="module")
def dev_ctx(yk):
    c = yk.Context(0)
    c.set_option("bvh_builder", 1)
    yield c
    c.close()


def _assert_device_built_equals_host(yk, dev_ctx, sd):
    ref = _tree(yk.Scene(None, sd))
    s = yk.Scene(dev_ctx, sd)
    bi = s.build_info()
    assert (bi.builder, bi.reason) == (DEVICE, 0), (bi.builder, bi.reason)  # the share of scenes allowed to leave the device path is zero
    got = _tree(s)
    s.close()
    assert got[2] == ref[2]
    assert got[0] == ref[0], "nodes differ"
    assert got[1] == ref[1], "shape order differs"
    return got, bi


@pytest.mark.parametrize("name", list(SCENES))
@pytest.mark.parametrize("method", [abi.SPLIT_SAH, abi.SPLIT_MIDDLE])
@pytest.mark.parametrize("max_shapes", [1, 4])
def test_device_built_tree_is_the_host_tree(yk, dev_ctx, name, method, max_shapes):
    sd = SCENES[name]()
    sd.split_method, sd.max_shapes_in_node = method, max_shapes
    got, bi = _assert_device_built_equals_host(yk, dev_ctx, sd)
    if (method, max_shapes) in TABLE[name]:
        assert (got[2][0], got[2][4]) == TABLE[name][(method, max_shapes)]


@pytest.mark.parametrize("small_range", [0, 2, 64, 1 << 20])
@pytest.mark.parametrize("method", [abi.SPLIT_SAH, abi.SPLIT_MIDDLE])
def test_every_small_range_limit_on_the_device(yk, method, small_range):
    """Each phase, and the seam between them, as the whole build: S = 0 the level kernels only, S above the scene's size one lane."""
    c = yk.Context(0, bvh_builder=1, bvh_small_range=small_range)
    one, dup = _one_and_seven()
    perm = scenes.by_name("city-tiny")
    perm.shape_order = np.random.default_rng(5).permutation(perm.n_triangles).astype(np.uint32)
    for sd in (scenes.by_name("cornell-tris"), scenes.by_name("city-tiny"), one, dup, perm, _signed_zero_scene()):
        for max_shapes in (1, 4):
            sd.split_method, sd.max_shapes_in_node = method, max_shapes
            _, bi = _assert_device_built_equals_host(yk, c, sd)
            assert bi.small_range == small_range
    c.close()


@pytest.mark.parametrize("k", [512, 513])
@pytest.mark.parametrize("method", [abi.SPLIT_SAH, abi.SPLIT_MIDDLE])
@pytest.mark.parametrize("max_shapes", [1, 4])
def test_compaction_at_the_scan_block_seam(yk, dev_ctx, k, method, max_shapes):
    """1024 and 1026 slots: one full block of the compaction's scan, then one full block and a tail of two."""
    sd = _seam_scene(k)
    sd.split_method, sd.max_shapes_in_node = method, max_shapes
    got, _ = _assert_device_built_equals_host(yk, dev_ctx, sd)
    assert got[2][0] == {(512, 1): 1023, (513, 1): 1025, (512, 4): 255, (513, 4): 257}[(k, max_shapes)]


def test_cornell_with_its_sphere(yk, dev_ctx):
    _assert_device_built_equals_host(yk, dev_ctx, scenes.cornell())


@pytest.mark.parametrize("method,max_shapes", [(abi.SPLIT_SAH, 1), (abi.SPLIT_SAH, 4), (abi.SPLIT_MIDDLE, 1)])
def test_cfg3_at_full_size(yk, dev_ctx, method, max_shapes):
    sd = scenes.by_name("cfg3")
    sd.split_method, sd.max_shapes_in_node = method, max_shapes
    got, _ = _assert_device_built_equals_host(yk, dev_ctx, sd)
    assert (got[2][0], got[2][4]) == {(abi.SPLIT_SAH, 1): (2035599, 27), (abi.SPLIT_SAH, 4): (646811, 25), (abi.SPLIT_MIDDLE, 1): (2048011, 29)}[(method, max_shapes)]


def test_cfg5(yk, dev_ctx):
    sd = scenes.by_name("cfg5")
    sd.split_method, sd.max_shapes_in_node = abi.SPLIT_SAH, 1
    got, _ = _assert_device_built_equals_host(yk, dev_ctx, sd)
    assert (got[2][0], got[2][4]) == (20354077, 30)


@pytest.mark.parametrize("wide", [0, 2])
def test_render_through_a_device_built_scene(yk, wide):
    """city-small, Path 6, both samplers, one tile list: the device records laid out from the device-built tree are the default's."""
    sd = scenes.by_name("city-small")
    fs = yk.FilmSettings(res=(160, 90), tile_dim=16)
    cam, tiles = yk.Camera(sd.camera, fs), yk.film_tiles(fs)
    integ = yk.IntegratorType.Path(yk.PathParams(max_depth=6))
    images = {}
    for builder in (0, 1):
        c = yk.Context(0, wide_bvh=wide, bvh_builder=builder)
        sc = yk.Scene(c, sd)
        assert sc.build_info().builder == builder and sc.build_info().reason == 0
        for k, sampler in enumerate((yk.SamplerType.Uniform(4, SEED), yk.SamplerType.Stratified((2, 2), True, SEED))):
            px, st = yk.IntegratorType.instantiate(c, integ).render_tiles(sc, cam, sampler, tiles)
            images[(builder, k)] = (np.ascontiguousarray(px, dtype=np.float32).view(np.uint32).copy(), st.rays)
        sc.close()
        c.close()
    for k in (0, 1):
        assert images[(0, k)][1] == images[(1, k)][1]
        assert np.array_equal(images[(0, k)][0], images[(1, k)][0])


def test_build_info_names_the_builder_and_nothing_is_left_behind(yk, oracle, dev_ctx):
    sd = scenes.by_name("city-tiny")
    plain = yk.Context(0)
    s = yk.Scene(plain, sd)
    assert (s.build_info().builder, s.build_info().reason) == (HOST, 0)  # without the option: the host recursion
    s.close()
    plain.close()
    eq = scenes.by_name("city-tiny")
    eq.split_method, eq.max_shapes_in_node = abi.SPLIT_EQUAL_COUNTS, 2
    s = yk.Scene(dev_ctx, eq)
    assert (s.build_info().builder, s.build_info().reason) == (HOST, REASON_SPLIT_METHOD)
    assert _tree(s)[:2] == _tree(yk.Scene(None, eq))[:2]
    s.close()
    # a second scene on the context after device builds renders as the oracle says
    first = yk.Scene(dev_ctx, scenes.by_name("city-small"))
    assert first.build_info().builder == DEVICE
    second = yk.Scene(dev_ctx, sd)
    assert second.build_info().builder == DEVICE
    fs = yk.FilmSettings(res=(96, 54), tile_dim=16)
    cam, tiles = yk.Camera(sd.camera, fs), yk.film_tiles(fs)
    sampler, integ = yk.SamplerType.Stratified((2, 2), True, SEED), yk.IntegratorType.Path(yk.PathParams(max_depth=6))
    got, st = yk.IntegratorType.instantiate(dev_ctx, integ).render_tiles(second, cam, sampler, tiles)
    want, rays = oracle.OracleScene(sd).render_tiles(cam.matrices, sampler, integ, tiles, n_threads=0)
    assert st.rays == rays
    assert np.array_equal(np.ascontiguousarray(got, dtype=np.float32).view(np.uint32), np.ascontiguousarray(want, dtype=np.float32).view(np.uint32))
    first.close()
    second.close()
