"""The one-lane brute-force kernels' shading rows (rt_kernels.hip render_kernel ROWS): in place of tri_shade's copy
and the material table they stage one row per triangle in LDS, n.xyz type | colour.xyz rough, built in the prologue from
the same global arrays, so that a shading look-up is one read.  The rows hold copies: every frame is the CPU oracle's,
bit for bit.

The scene: a closed room (tests/test_brute_shell.py wall_box) whose walls are diffuse, glossy and glass, with an
emitter quad under the ceiling and two small blocks.  Two walls share a material, two materials differ in `rough`
alone, and two more in colour alone: a row built from a neighbour's material, or from the wrong half of its own,
changes the frame.  The sun is on (env[3] > 0), so the sun term reads the surface's row and the occluder's.

1024 x 352 at 4 spp, maxBounce 4 (the tile at which the automatic clustered kernel runs, tests/test_gpu_brute_shell.py)
for the frame, four adds and a listed add; 64 x 64 with team = 1 for the lock-step one-lane kernel, and with team = 4
for the team kernel, which keeps the table."""
import types

import numpy as np
import pytest

import oracle.oracle as O
from ensem3a_openclraytracer_amd import _native
from ensem3a_openclraytracer_amd import workloads as W
from tests import test_gpu_brute_shell as S
from tests.test_brute_shell import UNIT, wall_box

pytestmark = pytest.mark.gpu

SPP, MB, SMALL, LARGE = S.SPP, S.MB, S.SMALL, S.LARGE
# type, colour, rough, ior.  1 / 2: equal but for rough; 0 / 5: equal but for colour; 3: glass; 4: the emitter
MATS = np.array([[1, 0.8, 0.7, 0.6, 0.0, 1.0], [2, 0.9, 0.9, 0.9, 0.25, 1.0], [2, 0.9, 0.9, 0.9, 0.6, 1.0],
                 [3, 0.95, 1.0, 1.0, 0.0, 1.5], [0, 1.0, 1.0, 1.0, 3.0, 1.0], [1, 0.2, 0.5, 0.9, 0.0, 1.0]], np.float32)
# Cornell at 1024 x 1024 (the benchmark's frame): grid and dynamic LDS bytes of the launch, read from
# rt_debug_last_launch on a build of the parent commit at 4 spp, as the test launches it (the clustered sliced
# kernel, 128 lanes per block; neither figure depends on spp: launch_pick sizes the grid by the tile's pixels and
# the resident blocks, the LDS by the scene)
PARENT_GRID, PARENT_LDS = 2560, 15072


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


def _quad(box):
    """The two triangles of the flat box `box` (lo.x hi.x lo.y hi.y lo.z hi.z), as tests/test_brute_shell.py
    room_scene cuts its walls."""
    w = np.asarray(box, np.float32)
    a = int(np.argmax(w[0::2] == w[1::2]))
    u, v = [k for k in range(3) if k != a]
    c = np.zeros((4, 3), np.float32)
    c[:, a] = w[2 * a]
    c[:, u] = [w[2 * u], w[2 * u + 1], w[2 * u + 1], w[2 * u]]
    c[:, v] = [w[2 * v], w[2 * v], w[2 * v + 1], w[2 * v + 1]]
    return [c[[0, 1, 2]], c[[0, 2, 3]]]


def room():
    from ensem3a_openclraytracer_amd import bvh as B
    rng = np.random.default_rng(2100)
    tris, mats = [], []
    # walls -x +x -y +y -z +z: diffuse, the same diffuse, glossy, the other glossy, glass, the other diffuse
    for f, m in enumerate((0, 0, 1, 2, 3, 5)):
        tris += _quad(wall_box(UNIT, f))
        mats += [m, m]
    tris += _quad((-0.3, 0.3, -0.3, 0.3, 0.9, 0.9))           # the emitter, under the ceiling
    mats += [4, 4]
    for k, centre in enumerate(([0.45, 0.3, -0.6], [-0.5, -0.2, -0.55])):
        for j in range(8):
            p = np.asarray(centre) + rng.uniform(-0.06, 0.06, 3)
            tris.append((p + rng.normal(0.0, 0.03, (3, 3))).astype(np.float32))
            mats.append((1, 2, 3, 5, 0, 2, 1, 3)[(j + 3 * k) % 8])
    tri = np.asarray(tris, np.float32)
    n = len(tri)
    vp = tri.reshape(-1, 3)
    nrm = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    nrm = (nrm / np.maximum(np.linalg.norm(nrm, axis=1, keepdims=True), 1e-20)).astype(np.float32)
    face = np.zeros((n, 10), np.int32)
    face[:, 0] = mats
    face[:, 4:7] = np.arange(n)[:, None]
    face[:, 7:10] = np.arange(3 * n).reshape(n, 3)
    fd = face.ravel()
    return types.SimpleNamespace(V_p=vp.ravel(), V_n=nrm.ravel(), V_uv=np.zeros(2, np.float32), faceData=fd,
                                 materialData=MATS.ravel(), lightData=np.zeros(0, np.float32), BVH=B.BVH(fd, vp.ravel()))


_scene, _refs = [], {}


def _inputs(size):
    if not _scene:
        _scene.append(room())
    _, cam, env = S._cornell()
    cam, env = cam.copy(), env.copy()
    cam[0:3] = [0.1, -0.8, 0.2]           # inside the closed room
    cam[3:6] = [8.0, -5.0, 0.0]
    env[3] = 2.0                           # the sun is on
    return _scene[0], S._sized(cam, size), env


def _want(size):
    if size not in _refs:
        sc, cam, env = _inputs(size)
        _refs[size] = O.render(O.OracleScene.from_scene(sc, W.ibl_preview()), cam, env, size[0] * size[1], SPP, MB,
                               nthreads=16)
    return _refs[size]


def _frame(kl, size, **opts):
    sc, cam, env = _inputs(size)
    for key, v in dict(S.DEFAULTS, **opts).items():
        kl.native.set_option(key, v)
    npix = size[0] * size[1]
    out = np.zeros(3 * npix, np.float32)
    kl.launch_Raytracing(out, sc.V_p, sc.V_n, sc.V_uv, sc.faceData, sc.materialData, sc.lightData,
                         sc.BVH.exportArray, cam, env, npix, SPP, MB, W.ibl_preview())
    assert kl.native.scene_info()["brute_records"] == len(sc.faceData) // 10
    return out, _native.last_launch()


def _progressive(kl, size):
    sc, cam, env = _inputs(size)
    return kl.begin_progressive(sc.V_p, sc.V_n, sc.V_uv, sc.faceData, sc.materialData, sc.lightData,
                                sc.BVH.exportArray, cam, env, size[0] * size[1], MB, W.ibl_preview())


def test_the_frame_sees_every_material_and_the_sun():
    """The oracle's frame itself: it changes with the sun, and with either of the materials that differ from
    another in one field alone -- so a wrong row would show."""
    sc, cam, env = _inputs(SMALL)
    want = _want(SMALL)
    assert np.isfinite(want).all() and want.std() > 0
    osc = O.OracleScene.from_scene(sc, W.ibl_preview())
    dark = env.copy()
    dark[3] = 0.0
    assert not np.array_equal(O.render(osc, cam, dark, SMALL[0] * SMALL[1], SPP, MB, nthreads=16), want)
    for m, field in ((2, 4), (5, 2)):
        other = types.SimpleNamespace(**vars(sc))
        md = sc.materialData.copy()
        md[6 * m + field] = MATS[m - 1 if m == 2 else 0, field]
        other.materialData = md
        got = O.render(O.OracleScene.from_scene(other, W.ibl_preview()), cam, env, SMALL[0] * SMALL[1], SPP, MB,
                       nthreads=16)
        assert not np.array_equal(got, want), (m, field)


def test_clustered_frame_four_adds_and_a_listed_add(kl):
    want = _want(LARGE)
    got, ll = _frame(kl, LARGE)
    assert ll["brute"] & 3 == 3, ll
    S._same(got, want, ll)
    p = _progressive(kl, LARGE)
    for n in (1, 1, 1, 1):
        got = p.add(n)
        ll = _native.last_launch()
        assert ll["acc"] == 1 and ll["brute"] & 3 == 3, ll
    p.close()
    S._same(got, want, "four adds")
    p = _progressive(kl, LARGE)
    p.add(2)
    p.select_all()
    got = p.add_selected(2)
    ll = _native.last_launch()
    assert ll["acc"] == 2 and ll["brute"] & 3 == 3, ll
    p.close()
    S._same(got, want, "listed add")


def test_lockstep_and_team_kernels(kl):
    want = _want(SMALL)
    for opts, family in ((dict(team=1), 1), (dict(team=1, brute_cluster=1), 3), (dict(team=4), 2)):
        got, ll = _frame(kl, SMALL, **opts)
        assert ll["brute"] & 3 == family, (opts, ll)
        S._same(got, want, opts)


def test_cornell_1024_launch_is_no_smaller_and_no_heavier_than_the_parents(kl):
    sc, cam, env, npix, _, mb, ibl = W.CONFIGS["C2"].inputs()
    assert npix == 1024 * 1024
    out = np.zeros(3 * npix, np.float32)
    kl.launch_Raytracing(out, sc.V_p, sc.V_n, sc.V_uv, sc.faceData, sc.materialData, sc.lightData,
                         sc.BVH.exportArray, cam, env, npix, 4, mb, ibl)
    ll = _native.last_launch()
    assert ll["brute"] & 3 == 3, ll
    assert ll["grid"] >= PARENT_GRID and ll["lds"] <= PARENT_LDS, ll
