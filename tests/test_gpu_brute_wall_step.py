"""The shell's one queue step on the GPU (rt_device.h trace_brute_compact; tests/test_brute_wall_step.py has what it
rests on): a wave whose lanes pass at most one face each queues the passes of all faces in one step, any other wave
queues them face by face.  Both give the frame of "brute_shell" = 0 (the walls as single slots, one step per slot),
bit for bit, and the CPU oracle's.

tests/test_gpu_brute_shell.py and tests/test_gpu_brute_near.py render Cornell from in front of its open side, from
inside, and with a non-finite camera.  The cases here are the ones a wave needs to take the per-face steps for every
primary ray, or to mix both kinds of lanes: a camera outside a closed room (in through one wall, out through
another), a camera on an edge of the room and one in a corner (two or three plane distances of 0), and a closed room
with a NaN in the camera's origin.  1024 x 352 at 4 spp, maxBounce 4: the tile at which the automatic clustered
kernel runs, as in tests/test_gpu_brute_shell.py."""
import numpy as np
import pytest

import oracle.oracle as O
from ensem3a_openclraytracer_amd import _native
from ensem3a_openclraytracer_amd import workloads as W
from tests import test_gpu_brute_shell as S
from tests.test_brute_shell import six_face_room

pytestmark = pytest.mark.gpu

SPP, MB, LARGE = S.SPP, S.MB, S.LARGE
CASES = ["closed_room_from_outside", "cornell_on_an_edge", "cornell_in_a_corner", "closed_room_cam_nan"]
_refs = {}


@pytest.fixture(scope="module")
def kl():
    from ensem3a_openclraytracer_amd.KernelLauncher import KernelLauncher
    k = KernelLauncher(None, None, 0, None)
    yield k
    for key, v in S.DEFAULTS.items():
        k.native.set_option(key, v)
    k.close()


@pytest.fixture(autouse=True)
def _defaults(kl):
    yield
    for key, v in S.DEFAULTS.items():
        kl.native.set_option(key, v)


def _case(name):
    sc, cam, env = S._cornell()
    cam = cam.copy()
    if name == "closed_room_from_outside":
        sc = six_face_room()                     # cam at (0, -3.5, 0) looking at the -y wall from outside
    elif name == "cornell_on_an_edge":
        cam[0:3] = [-1.0, -0.9, -1.0]            # on the edge of the -x and -z walls, looking into the room
        cam[3:6] = [30.0, 0.0, -40.0]
    elif name == "cornell_in_a_corner":
        cam[0:3] = [-1.0, -1.0, -1.0]            # ... of those two and the open front
        cam[3:6] = [0.0, 0.0, -40.0]
    else:
        assert name == "closed_room_cam_nan"
        sc = six_face_room()
        cam[0:3] = [0.1, S.NAN, 0.2]
    return sc, S._sized(cam, LARGE), env


def _want(name):
    if name not in _refs:
        sc, cam, env = _case(name)
        _refs[name] = O.render(O.OracleScene.from_scene(sc, W.ibl_preview()), cam, env, LARGE[0] * LARGE[1], SPP, MB,
                               nthreads=16)
    return _refs[name]


def _frame(kl, name, **opts):
    sc, cam, env = _case(name)
    for key, v in dict(S.DEFAULTS, **opts).items():
        kl.native.set_option(key, v)
    npix = LARGE[0] * LARGE[1]
    out = np.zeros(3 * npix, np.float32)
    kl.launch_Raytracing(out, sc.V_p, sc.V_n, sc.V_uv, sc.faceData, sc.materialData, sc.lightData,
                         sc.BVH.exportArray, cam, env, npix, SPP, MB, W.ibl_preview())
    return out, _native.last_launch()


def _progressive(kl, name):
    sc, cam, env = _case(name)
    return kl.begin_progressive(sc.V_p, sc.V_n, sc.V_uv, sc.faceData, sc.materialData, sc.lightData,
                                sc.BVH.exportArray, cam, env, LARGE[0] * LARGE[1], MB, W.ibl_preview())


@pytest.mark.parametrize("name", CASES)
def test_one_shot_equals_the_single_slots_and_the_oracle(kl, name):
    off, ll = _frame(kl, name, brute_shell=0)
    assert ll["brute"] & 3 == 3 and ll["shell"] == 0
    S._same(off, _want(name), name)
    got, ll = _frame(kl, name)
    assert ll["brute"] & 3 == 3 and ll["shell"] == 1, ll
    S._same(got, off, name)


@pytest.mark.parametrize("name", CASES)
def test_four_adds_and_a_listed_add_equal_the_oracle(kl, name):
    """The rt_accum and rt_adaptive instantiations: 1 + 1 + 1 + 1 samples; 2 samples, then 2 more through the list."""
    p = _progressive(kl, name)
    for n in (1, 1, 1, 1):
        got = p.add(n)
        ll = _native.last_launch()
        assert ll["acc"] == 1 and ll["brute"] & 3 == 3 and ll["shell"] == 1, ll
    p.close()
    S._same(got, _want(name), name)
    p = _progressive(kl, name)
    p.add(2)
    p.select_all()
    got = p.add_selected(2)
    ll = _native.last_launch()
    assert ll["acc"] == 2 and ll["brute"] & 3 == 3 and ll["shell"] == 1, ll
    p.close()
    S._same(got, _want(name), name)
