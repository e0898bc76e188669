"""Scenes, cameras and comparisons of the radiance-query tests (tests/test_gpu_radiance.py).

cornell and caterpillar are tests/test_gpu_nonfinite.py's; the seeded soups are built here the way
tests/test_gpu_parity.py builds its random scenes (the builder below is a copy: all four material types, degenerate
triangles, ties), 7 triangles for the brute force and 150 for the BVH2 walk.  Every frame is 25 x 23 pixels: 575
rays, a partial last wave and a partial block at every block size.
"""
import functools
import types

import numpy as np

import oracle.oracle as O
from ensem3a_openclraytracer_amd import workloads as W

WIDTH, HEIGHT = 25, 23
NPIX = WIDTH * HEIGHT
SPP = 5
BOUNCES = (-1, 0, 1, 4)
# sun power and IBL power, each zero and non-zero
POWERS = ((0.5, 0.3), (0.0, 0.3), (0.5, 0.0), (0.0, 0.0))
SCENES = ("cornell", "soup7", "soup150", "caterpillar")


def random_scene(seed, ntri):
    from ensem3a_openclraytracer_amd import bvh as B
    rng = np.random.default_rng(1000 + seed)
    # odd seeds: the soup around the camera (0, -3.5, 0), so camera rays start inside boxes and between triangles
    c = rng.uniform(-1.5, 1.5, (ntri, 1, 3)) + np.array([0.0, -3.5 if seed % 2 else 1.0, 0.0])
    tri = c + rng.normal(0.0, 0.35, (ntri, 3, 3)) * rng.choice([0.05, 0.4, 1.0], (ntri, 1, 1))
    k = max(1, ntri // 10)
    tri[:k, 2] = tri[:k, 1]                                                        # zero-area (two equal corners)
    tri[k:2 * k, 2] = 0.5 * (tri[k:2 * k, 0] + tri[k:2 * k, 1])                     # collinear
    tri[2 * k:3 * k] = tri[3 * k:4 * k] + np.array([1.0 / 64, 0.0, 0.0])              # overlapping shifted copies
    if ntri >= 8:
        tri[4 * k:4 * k + 1] *= 8.0                                                # a huge one
    tri[5 * k:6 * k, :, 2] = np.round(tri[5 * k:6 * k, :, 2])                       # coplanar on z = integer
    tri = np.round(tri.astype(np.float32) * 64) / 64                               # shared coordinates: ties
    vp = tri.reshape(-1, 3).astype(np.float32)
    nrm = rng.normal(size=(ntri, 3)).astype(np.float32)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    vn = nrm.astype(np.float32)
    nmat = 5
    mat = np.array([[1, 0.8, 0.7, 0.6, 0.0, 1.0],      # diffuse
                    [2, 0.9, 0.9, 0.9, 0.25, 1.0],     # glossy
                    [3, 0.95, 1.0, 1.0, 0.0, 1.5],     # glass
                    [0, 1.0, 1.0, 1.0, 3.0, 1.0],      # emitter (emission = roughness)
                    [1, 0.2, 0.5, 0.9, 0.0, 1.0]], np.float32)
    face = np.zeros((ntri, 10), np.int32)
    face[:, 0] = rng.integers(0, nmat, ntri)
    face[:, 4:7] = np.arange(ntri)[:, None]
    face[:, 7:10] = np.arange(3 * ntri).reshape(ntri, 3)
    fd = face.ravel()
    return types.SimpleNamespace(V_p=vp.ravel(), V_n=vn.ravel(), V_uv=np.zeros(2, np.float32), faceData=fd,
                                 materialData=mat.ravel(), lightData=np.zeros(0, np.float32), BVH=B.BVH(fd, vp.ravel()))


def _frame_cam(cam):
    cam = np.array(cam, np.float32)
    cam[6], cam[7] = WIDTH, HEIGHT
    return cam


@functools.lru_cache(maxsize=None)
def scene(name):
    """A namespace with the scene arrays, ``bvh``, ``options`` (the rt_set_option values it is rendered with),
    ``cam`` (a 25 x 23 frame) and ``env``."""
    if name in ("cornell", "caterpillar"):
        from tests.test_gpu_nonfinite import scene as nonfinite_scene
        sc = nonfinite_scene(name)
        return types.SimpleNamespace(V_p=sc.V_p, V_n=sc.V_n, V_uv=sc.V_uv, faceData=sc.faceData,
                                     materialData=sc.materialData, lightData=sc.lightData, bvh=sc.bvh, name=name,
                                     options=dict(sc.options), cam=_frame_cam(sc.cam), env=np.array(sc.env, np.float32))
    seed, ntri = {"soup7": (19, 7), "soup150": (3, 150)}[name]
    sc = random_scene(seed, ntri)
    cam = np.array([0.0, -3.5, 0.0, 16.0, 12.0, 0.0, WIDTH, HEIGHT, 1, 25.0 * (3.14 / 180)], np.float64)
    if name == "soup7":   # a wide view from inside the soup: a diffuse and a glass triangle in 102 of the 575 pixels
        cam[3:6], cam[9] = 0.0, 100.0 * (3.14 / 180)
    return types.SimpleNamespace(V_p=sc.V_p, V_n=sc.V_n, V_uv=sc.V_uv, faceData=sc.faceData,
                                 materialData=sc.materialData, lightData=sc.lightData,
                                 bvh=np.array(sc.BVH.exportArray, np.float32), name=name, options={},
                                 cam=cam.astype(np.float32), env=np.array([60.0, -30.0, 10.0, 0.5, 0.3], np.float32))


def ntri(sc):
    return sc.faceData.size // 10


def env_with(sc, sun, ibl):
    env = np.array(sc.env, np.float32)
    env[3], env[4] = sun, ibl
    return env


@functools.lru_cache(maxsize=None)
def oracle_scene(name, shallow=False):
    """shallow: the same triangles in the tree BVH.py builds for them -- the FAST reference of caterpillar, whose
    own chain overflows the reference's 20-slot stack (REF drops with it, FAST has no cap)."""
    sc = scene(name)
    bvh = sc.bvh
    if shallow:
        from ensem3a_openclraytracer_amd import bvh as B
        bvh = B.build_export_array(sc.faceData, sc.V_p)
    return O.OracleScene(sc.V_p, sc.V_n, sc.V_uv, sc.faceData, sc.materialData, bvh, W.ibl_preview())


def oracle_rays(cam, npix, first=0, count=None):
    """The reference's camera rays of pixels first .. first + count - 1 as rt_camera_rays packs them: float32
    [count, 8] = genCameraRay's (dir, origin), then the seed words (i % npix, i / npix)."""
    count = npix - first if count is None else count
    rays = np.zeros((count, 8), np.float32)
    for t in range(count):
        rays[t, :6] = O.camera_ray(cam, first + t)
    rays.view(np.uint32)[:, 6] = (np.arange(first, first + count) % npix).astype(np.uint32)
    rays.view(np.uint32)[:, 7] = (np.arange(first, first + count) // npix).astype(np.uint32)
    return rays


def oracle_frame(name, cam, env, npix, spp, max_bounce, shallow=False):
    return O.render(oracle_scene(name, shallow), cam, env, npix, spp, max_bounce, nthreads=16).reshape(-1, 3)[:npix]


def clamp(rgb):
    """Raytracing.cl:211-220 on an unclamped mean: fmax(fmin(x, 1), 0), which sends NaN to 1."""
    return np.fmax(np.fmin(np.asarray(rgb, np.float32), np.float32(1.0)), np.float32(0.0))


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def differing(a, b):
    """Rows whose floats are not the same bits (NaN equal to NaN)."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    same = (bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))
    return np.nonzero(~same.reshape(len(a), -1).all(1))[0]
