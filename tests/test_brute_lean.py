"""Option "brute_lean" on the host (rt_debug.h rt_debug_brute_lean; scene_pack.cpp materials_diffuse_only, rt_internal.h
brute_lean_frame / brute_lean_kernel): the packer's census of the material types and the rule by which launch_pick
takes the lean form of a one-lane brute-force kernel.  No device: tests/test_gpu_brute_lean.py has the kernels."""
import numpy as np
import pytest

from ensem3a_openclraytracer_amd import _native

ENV = np.array([10.0, 20.0, 30.0, 1.5, 0.0], np.float32)   # a lit sun, no IBL power


def table(*types):
    """A material table of rows type | colour | rough | unused, as FileManager packs them."""
    return np.array([[t, 0.5, 0.25, 0.75, 2.0, 0.0] for t in types], np.float32).reshape(-1)


def lean(mat=None, env=ENV, **kw):
    return _native.brute_lean(table(1, 1, 0, 1) if mat is None else mat, env, **kw)


@pytest.mark.parametrize("types,want", [
    ((1, 1, 1), True),            # all diffuse
    ((1, 0, 1, 1), True),         # an emitter among them
    ((1, 2, 1), False),           # one glossy
    ((1, 1, 3), False),           # one glass
    ((), True),                   # an empty table holds no other type
    ((0,), True),
    ((1.75, 0.5, -0.5), True),    # the kernels read (int)type: these are 1, 0 and 0
    ((2.0,), False),
    ((np.nan,), False),
])
def test_census_of_the_material_types(types, want):
    only, _ = _native.brute_lean(table(*types), ENV)
    assert only is want


def test_cornell_is_diffuse_only():
    from ensem3a_openclraytracer_amd import workloads as W
    sc, cam, env, *_ = W.CONFIGS["C2"].inputs()
    types = sorted(np.asarray(sc.materialData, np.float32).reshape(-1, 6)[:, 0].astype(int).tolist())
    assert types == [0, 1, 1, 1]
    assert _native.brute_lean(sc.materialData, env) == (True, True)


def test_the_rule_holds_with_everything_on():
    for loop in (1, 3):
        for option in (-1, 1):
            assert lean(loop=loop, option=option) == (True, True)
    assert lean(spp=1, max_bounce=0) == (True, True)
    assert lean(env=np.array([0, 0, 0, 0.0, 0.0], np.float32)) == (True, True)       # an unlit sun (sun_skip) as well
    assert lean(env=np.array([0, 0, 0, -0.0, 0.0], np.float32)) == (True, True)      # e3 = -0: the kernel keeps its add


@pytest.mark.parametrize("off", [
    dict(option=0),
    dict(mat=table(1, 2)), dict(mat=table(3, 1)),
    dict(env=np.array([10, 20, 30, 1.5, 0.5], np.float32)),
    dict(env=np.array([10, 20, 30, 1.5, -0.0], np.float32)),      # -0 is zero to sample_ibl_if, not to the lean loop's bits
    dict(env=np.array([10, 20, 30, 1.5, np.nan], np.float32)),
    dict(pass_=1), dict(pass_=2), dict(pilot=2),
    dict(spp=0), dict(max_bounce=-1),
    dict(fixed_point=0), dict(sun_cache=0),
    dict(loop=0), dict(loop=2), dict(loop=1, team=4),             # a tree walk, the team kernel
    dict(count=1), dict(log=1), dict(acc=1), dict(acc=2),         # instrumented, logging, an add, a listed add
    dict(traversal=1),
])
def test_each_condition_switched_off_in_turn(off):
    only, on = lean(**off)
    assert on is False
    assert only is ("mat" not in off)


def test_bad_arguments():
    for bad in (-2, 2):
        with pytest.raises(_native.NativeError):
            lean(option=bad)
    with pytest.raises(_native.NativeError):
        _native.brute_lean(np.zeros(7, np.float32), ENV)          # not whole rows
