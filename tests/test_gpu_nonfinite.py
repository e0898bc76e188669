"""Non-finite rays through the GPU engines: NaN, infinite, zero and denormal ray components, far-away
origins, and frames whose camera, environment, normals, materials or vertices hold NaN / inf.

The expected output is well defined: the oracle (oracle/rt_oracle.c) and the kernels share rtm.h
(NaN-dropping fmin / fmax, a saturating float -> int, a clamp that turns NaN into 1), so the oracle's
frame is the reference of every case; REF must equal it bit for bit and FAST must too (NaN payloads
aside: numpy's array equality takes NaN == NaN).

What such rays do in the box tests (rt_device.h slab / box_hit drop NaN operands):
  * brute force (scenes of <= 64 triangles): a ray with a NaN component passes EVERY box slot, padding
    slots included -- the worst case of the pair queue; the padding slots list record 0
    (tests/test_malformed_inputs.py checks the layout on the host);
  * tree walks: fast_init's root test is !(tmax >= tmin && tmax >= 0), false for NaN distances, so a ray
    whose three axes all drop out ends at the root without a fetch; a stack entry whose entry distance is
    NaN is discarded when popped (NaN <= cull is false) -- harmless, such a ray can hit nothing;
  * the rays that do fill a traversal stack to its computed bound pass every box with a non-NaN entry
    distance: direction (+-inf, +-inf, +-inf) (every slab distance is +-0; single rays), and in frames a
    finite camera beside the caterpillar's triangles and inside all its boxes.
"""
import functools
import types

import numpy as np
import pytest

import oracle.oracle as O
from ensem3a_openclraytracer_amd import _native
from ensem3a_openclraytracer_amd import workloads as W
from tests import nonfinite_rays as NR
from tests.deep_bvh import caterpillar_scene
from tests.test_gpu_parity import _random_scene

pytestmark = pytest.mark.gpu

NAN, INF = np.float32(np.nan), np.float32(np.inf)
VN_NAN_OFFSET = 6   # which triangles of every seven take the NaN normal
NPIX, SPP, MB = 32 * 32, 4, 4
FIELDS = ("V_p", "V_n", "V_uv", "faceData", "materialData", "lightData")


@pytest.fixture(scope="module")
def kl():
    from ensem3a_openclraytracer_amd.KernelLauncher import KernelLauncher
    k = KernelLauncher(None, None, 0, None)
    yield k
    k.close()


# ---- scenes ----

def _ns(sc, **changes):
    d = {f: np.array(getattr(sc, f), copy=True) for f in FIELDS}
    d["bvh"] = np.array(sc.BVH.exportArray if hasattr(sc, "BVH") else sc.bvh, copy=True)
    d["name"], d["options"], d["cam"], d["env"] = sc.name, dict(sc.options), sc.cam.copy(), sc.env.copy()
    d.update(changes)
    return types.SimpleNamespace(**d, BVH=types.SimpleNamespace(exportArray=d["bvh"]))


SOUP_CAM = np.array([0.0, -3.5, 0.0, 16.0, 12.0, 0.0, 32, 32, 1, 25.0 * (3.14 / 180)], np.float64).astype(np.float32)
SOUP_ENV = np.array([60.0, -30.0, 10.0, 0.5, 0.3], np.float32)


@functools.lru_cache(maxsize=None)
def scene(name):
    """cornell (brute force, 22 boxes: 2 padding slots), soup5 (brute force), soup150 / soup2000 (BVH2 and
    4-wide, deeper than stack_lds = 8), caterpillar (40 triangles in a chain of 39 internal nodes, walked as
    built -- bvh = reference, no brute force: FAST depth 39, beyond the 20 LDS entries), monkey (single rays
    only).  sc.options: the rt_set_option values the scene is rendered with."""
    if name in ("cornell", "monkey"):
        wl = W.PARITY_CASES["cornell_64_s4" if name == "cornell" else "monkey_c3_64_s4"].with_size(32, 32, SPP)
        sc, cam, env, *_ = wl.inputs()
        sc.name, sc.options, sc.cam, sc.env = name, {}, np.asarray(cam, np.float32), np.asarray(env, np.float32)
        return _ns(sc)
    if name == "caterpillar":
        a = caterpillar_scene(40)
        sc = types.SimpleNamespace(**{f: a.get(f, np.zeros(0, np.float32)) for f in FIELDS}, bvh=a["bvh"],
                                   name=name, options={"bvh": _native.RT_BVH_REFERENCE, "brute_max": 0},
                                   cam=np.array([0, -3.5, 0, 0, 0, 0, 32, 32, 1, 45 * 3.14 / 180], np.float32),
                                   env=np.array([90, 0, 0, 1.0, 1.0], np.float32))
        return _ns(sc)
    seed, ntri = {"soup5": (20, 5), "soup150": (3, 150), "soup2000": (11, 2000)}[name]
    sc = _random_scene(seed, ntri)
    sc.name, sc.options, sc.cam, sc.env = name, {}, SOUP_CAM, SOUP_ENV
    return _ns(sc)


FRAME_SCENES = ["cornell", "soup5", "soup150", "soup2000", "caterpillar"]


def _ntri(sc):
    return sc.faceData.size // 10


def _per_triangle_normals(sc):
    """The scene with one normal per triangle (its first vertex's, the one the kernels shade with)."""
    face = sc.faceData.reshape(-1, 10).copy()
    vn = sc.V_n.reshape(-1, 3)[face[:, 4]].copy()
    face[:, 4:7] = np.arange(len(face))[:, None]
    return _ns(sc, V_n=vn.ravel(), faceData=face.ravel())


def _with_glossy_and_glass(sc):
    """The scene with a glossy (type 2) and a glass (type 3) material in use: where the material set lacks
    one it is appended, and every fourth triangle of the most used material takes it."""
    mat = sc.materialData.reshape(-1, 6).copy()
    face = sc.faceData.reshape(-1, 10).copy()
    idx = np.nonzero(face[:, 0] == np.argmax(np.bincount(face[:, 0])))[0]
    for k, row in ((2, [2, 0.9, 0.9, 0.9, 0.25, 1.0]), (3, [3, 0.95, 1.0, 1.0, 0.0, 1.5])):
        if not (mat[:, 0] == k).any():
            mat = np.concatenate([mat, np.array([row], np.float32)])
            face[idx[k - 1::4], 0] = len(mat) - 1
    return _ns(sc, materialData=mat.ravel(), faceData=face.ravel())


def _most_seen_triangles(sc, n):
    """The n triangles the clean scene's camera rays hit most (by a brute-force float64 test: only used
    to choose which vertices to poison)."""
    vp = sc.V_p.reshape(-1, 3).astype(np.float64)
    f = sc.faceData.reshape(-1, 10)
    a, e1, e2 = vp[f[:, 7]], vp[f[:, 8]] - vp[f[:, 7]], vp[f[:, 9]] - vp[f[:, 7]]
    seen = np.zeros(len(f), np.int64)
    for i in range(0, NPIX, 3):
        r = O.camera_ray(sc.cam, i).astype(np.float64)
        d, o = r[:3], r[3:]
        h = np.cross(d, e2)
        det = (e1 * h).sum(1)
        with np.errstate(all="ignore"):
            inv = 1.0 / det
            s = o - a
            u = inv * (s * h).sum(1)
            q = np.cross(s, e1)
            v = inv * (q @ d)
            k = inv * (e2 * q).sum(1)
            ok = (np.abs(det) > 1e-7) & (u >= 0) & (u <= 1) & (v >= 0) & (u + v <= 1) & (k > 1e-4)
        if ok.any():
            seen[np.nonzero(ok)[0][np.argmin(k[ok])]] += 1
    return np.argsort(-seen)[:n]


CAMERA_CASES = ["cam_pos_nan_1", "cam_pos_nan_all", "cam_pos_inf", "cam_pos_1e30", "cam3_nan", "cam9_nan", "cam9_zero"]
ENV_CASES = ["env0_nan", "env3_nan", "env3_inf", "env4_nan", "env4_inf", "env4_negative"]
PARTIAL_CASES = ["vn_zero_every_3rd", "vn_nan_every_7th", "mat_colour_nan", "mat_colour_inf", "roughness_zero",
                 "roughness_nan", "ior_zero", "ior_nan", "vertices_nan_after_bvh", "vertices_inf_after_bvh"]


@functools.lru_cache(maxsize=None)
def poisoned(name, case):
    """(clean scene or None, poisoned scene).  The clean scene is given for the partial cases: the scene the
    poison is applied to (same arrays but for the poison)."""
    sc = scene(name)
    cam, env = sc.cam.copy(), sc.env.copy()
    if case in CAMERA_CASES or case in ENV_CASES:
        if case == "cam_pos_nan_1": cam[0] = NAN
        elif case == "cam_pos_nan_all": cam[0:3] = NAN
        elif case == "cam_pos_inf": cam[0:3] = INF
        elif case == "cam_pos_1e30": cam[0:3] = np.float32(1e30)
        elif case == "cam3_nan": cam[3] = NAN
        elif case == "cam9_nan": cam[9] = NAN
        elif case == "cam9_zero": cam[9] = 0.0          # tan(0) = 0: the focal point is at infinity
        elif case == "env0_nan": env[0] = NAN
        elif case == "env3_nan": env[3] = NAN
        elif case == "env3_inf": env[3] = INF
        elif case == "env4_nan": env[4] = NAN
        elif case == "env4_inf": env[4] = INF
        elif case == "env4_negative": env[4] = -0.5
        return None, _ns(sc, cam=cam, env=env)
    if case.startswith("vn_"):
        clean = _per_triangle_normals(sc)
        vn = clean.V_n.reshape(-1, 3).copy()
        if case == "vn_zero_every_3rd": vn[0::3] = 0.0     # normalises to NaN: NaN bounce directions
        else: vn[VN_NAN_OFFSET::7] = NAN
        return clean, _ns(clean, V_n=vn.ravel())
    if case.startswith("vertices_"):
        # index-valid arrays rt_set_scene accepts: the BVH was built from the clean vertices
        vp = sc.V_p.reshape(-1, 3).copy()
        tri = _most_seen_triangles(sc, 3)
        rows = sc.faceData.reshape(-1, 10)[tri, 7 + np.arange(3) % 3]
        vp[rows] = NAN if case == "vertices_nan_after_bvh" else [INF, -INF, INF]
        return sc, _ns(sc, V_p=vp.ravel())
    clean = _with_glossy_and_glass(sc)
    mat = clean.materialData.reshape(-1, 6).copy()
    used = np.bincount(clean.faceData.reshape(-1, 10)[:, 0], minlength=len(mat))
    if case.startswith("mat_colour"):
        m = [i for i in np.argsort(-used) if mat[i, 0] == 1][0]      # the most used diffuse material
        mat[m, 2] = NAN if case == "mat_colour_nan" else INF
    elif case.startswith("roughness"):
        mat[np.nonzero(mat[:, 0] == 2)[0][0], 4] = 0.0 if case == "roughness_zero" else NAN
    else:
        mat[np.nonzero(mat[:, 0] == 3)[0][0], 5] = 0.0 if case == "ior_zero" else NAN
    return clean, _ns(clean, materialData=mat.ravel())


def oracle_frame(sc, spp=SPP, counts=False):
    osc = O.OracleScene(sc.V_p, sc.V_n, sc.V_uv, sc.faceData, sc.materialData, sc.bvh, W.ibl_preview())
    return O.render(osc, sc.cam, sc.env, NPIX, spp, MB, nthreads=16, counts=counts)


def pixels_differing(a, b):
    """Pixels whose three floats are not the same values (NaN equal to NaN)."""
    a, b = a.reshape(-1, 3), b.reshape(-1, 3)
    same = (a == b) | (np.isnan(a) & np.isnan(b))
    return np.nonzero(~same.all(1))[0]


# ---- GPU helpers ----

DEFAULTS = {"bvh": _native.RT_BVH_SAH, "brute_max": 64, "bvh_width": 0, "walk_team": 0, "team": 0, "stack_lds": 0, "fixed_point": 1,
            "sun_cache": 1, "sun_skip": 1, "pilot": -1, "spec": -1, "slices": -1, "resume_min": -1, "step": 0, "wdq": 1}


class options_set:
    """rt_set_option values for the length of a with block (the scene's own, then the given ones)."""

    def __init__(self, kl, sc, options):
        self.ctx, self.options = kl.native, {**sc.options, **options}

    def __enter__(self):
        for k, v in self.options.items():
            self.ctx.set_option(k, v)

    def __exit__(self, *exc):
        for k in self.options:
            self.ctx.set_option(k, DEFAULTS[k])


def render(kl, sc, traversal="fast", spp=SPP, **options):
    """One frame of sc with the given debug options (rt_debug.h), which are put back afterwards."""
    kl.set_traversal(traversal)
    out = np.zeros(3 * NPIX, np.float32)
    with options_set(kl, sc, options):
        kl.launch_Raytracing(out, sc.V_p, sc.V_n, sc.V_uv, sc.faceData, sc.materialData, sc.lightData, sc.bvh,
                             sc.cam, sc.env, NPIX, spp, MB, W.ibl_preview())
    return out


def count(kl, sc, traversal="fast", **options):
    """rt_count_work of one frame of sc, and the scene facts, under the given options."""
    render(kl, sc, traversal, **options)          # uploads the scene
    with options_set(kl, sc, options):
        return kl.native.count_work(sc.cam, sc.env, NPIX, SPP, MB), kl.native.scene_info()


def other_fast_paths(sc):
    """The FAST paths that must agree bit for bit with the default one.  The larger scene here is soup150:
    16.7 KB of nodes and triangles at depth 10 (wide depth 14), which the default 20-entry LDS stack lets
    choose_kernel stage in LDS (the SMEM kernels, BVH2 only -- bvh_width 4 alone would be that same kernel, so
    it is not listed).  stack_lds 8 is below its depth: the scene then walks global memory with the overflow
    buffer, the kernels of larger scenes, and only then does bvh_width 4 reach the 4-wide walk."""
    if _ntri(sc) <= 64:
        return {"tree walk, staged in LDS": dict(brute_max=0), "brute force, team 2": dict(team=2),
                "brute force, team 4": dict(team=4)}
    assert _ntri(sc) == 150
    return {"BVH2 staged in LDS": dict(bvh_width=2),
            "BVH2 staged in LDS, walk_team 2": dict(bvh_width=2, walk_team=2),
            "BVH2 staged in LDS, walk_team 4": dict(bvh_width=2, walk_team=4),
            "BVH2 in global memory with overflow (stack_lds 8)": dict(bvh_width=2, stack_lds=8),
            "BVH2 in global memory, walk_team 2": dict(bvh_width=2, stack_lds=8, walk_team=2),
            "BVH2 in global memory, walk_team 4": dict(bvh_width=2, stack_lds=8, walk_team=4),
            "4-wide walk (global memory, stack_lds 8)": dict(bvh_width=4, stack_lds=8),
            "4-wide walk without origin-folded dequantisation": dict(bvh_width=4, stack_lds=8, wdq=0)}


# FAST pixels that differ from the oracle through the documented slab rounding, (b - o) * (1 / d) against the
# reference's (b - o) / d, by (scene, case): each traced with rt_debug_pixel_log against
# oracle.pixel_log.  None so far; never more than NPIX // 100 per case.
PINNED = {}


def check_frame(kl, name, case, sc, want):
    ref = render(kl, sc, "ref")
    np.testing.assert_array_equal(ref, want, err_msg=f"{name} {case}: REF vs oracle")
    fast = render(kl, sc, "fast")
    diff = pixels_differing(fast, want)
    pinned = PINNED.get((name, case), [])
    assert len(pinned) <= NPIX // 100
    if len(diff):
        print(f"{name} {case}: FAST differs from the oracle on pixels {diff.tolist()[:40]} ({len(diff)})")
    assert diff.tolist() == sorted(pinned), (name, case, diff[:20])
    return fast


# ---- (a) single rays ----

RAY_SCENES = ["cornell", "soup5", "monkey", "soup150", "soup2000", "caterpillar"]


@functools.lru_cache(maxsize=None)
def rays_and_oracle(name):
    sc = scene(name)
    leaf = sc.bvh.reshape(-1, 9)
    leaf = leaf[leaf[:, 8] >= 0][:, 2:8]
    classes = NR.ray_classes(sc.cam[:3], leaf, seed=len(name), per_class=9)
    rng = np.random.default_rng(77)
    signs = rng.choice([-1.0, 1.0], (12, 3)).astype(np.float32)
    o = np.tile(sc.cam[:3], (12, 1)) + rng.uniform(-0.5, 0.5, (12, 3)).astype(np.float32)
    # passes every box with entry distance +-0: the ray that fills the traversal stacks to their bound
    classes["inf_dir_all"] = np.concatenate([signs * INF, o], axis=1).astype(np.float32)
    rays = np.concatenate(list(classes.values()))
    names = [k for k, v in classes.items() for _ in range(len(v))]
    osc = O.OracleScene(sc.V_p, sc.V_n, sc.V_uv, sc.faceData, sc.materialData, sc.bvh, W.ibl_preview())
    want = np.array([O.trace(osc, r) for r in rays])
    want_fast = want
    if name == "caterpillar":
        # the reference's 20-slot stack drops the nearest triangles of this 40-level chain (and REF drops them
        # with it, test_gpu_parity.py test_ref_stack_overflow_drops_like_the_reference); FAST has no cap, so its
        # reference is the oracle over the same triangles in the shallow tree BVH.py builds for them (the same
        # exact leaf boxes, no drop)
        from ensem3a_openclraytracer_amd import bvh as B
        shallow = O.OracleScene(sc.V_p, sc.V_n, sc.V_uv, sc.faceData, sc.materialData,
                                B.build_export_array(sc.faceData, sc.V_p), W.ibl_preview())
        want_fast = np.array([O.trace(shallow, r) for r in rays])
        assert (want_fast[:, 3] != want[:, 3]).any()
    return rays, names, want, want_fast


@pytest.mark.parametrize("traversal", ["ref", "fast"])
@pytest.mark.parametrize("name", RAY_SCENES)
def test_single_rays_match_oracle(kl, name, traversal):
    """rt_debug_trace against oracle.trace over the ray classes of tests/nonfinite_rays.py: the hit flag, the
    bits of k and the hit's material.  FAST is the brute force on cornell and soup5 (every NaN ray passes
    every slot, padding included) and the plain BVH2 walk with its whole stack in LDS on the others (exactly
    `depth` entries: the caterpillar's 39, which the inf_dir_all rays fill)."""
    sc = scene(name)
    rays, names, want, want_fast = rays_and_oracle(name)
    if traversal == "fast":
        want = want_fast
    assert 150 <= len(rays) <= 260
    ctx = kl.native
    render(kl, sc, traversal)                     # uploads the scene through the launcher
    with options_set(kl, sc, {}):
        info = ctx.scene_info()
        assert info["fast_ok"]
        if traversal == "fast":      # (the facts are those of the traversal in use)
            assert (info["brute_records"] > 0) == (name in ("cornell", "soup5"))
        if name == "caterpillar":
            assert info["depth"] == 39
        got = ctx.debug_trace(rays, _native.RT_TRAVERSAL_REF if traversal == "ref" else _native.RT_TRAVERSAL_FAST)
    hit = got[:, 1] >= 0
    bad = np.nonzero(hit != (want[:, 5] == 1))[0]
    assert not len(bad), [(names[i], rays[i].tolist(), got[i].tolist(), want[i, 3:6].tolist()) for i in bad[:5]]
    assert hit.any() and not hit.all()
    bad = np.nonzero(got[hit, 0].view(np.uint32) != want[hit, 3].astype(np.float32).view(np.uint32))[0]
    assert not len(bad), [(names[np.nonzero(hit)[0][i]], got[hit][i].tolist(), want[hit][i, 3]) for i in bad[:5]]
    mats = sc.faceData.reshape(-1, 10)[got[hit, 1].astype(int), 0]
    np.testing.assert_array_equal(mats, want[hit, 4])


# ---- (b) poisoned frames ----

@pytest.mark.parametrize("case", CAMERA_CASES)
@pytest.mark.parametrize("name", FRAME_SCENES)
def test_poisoned_camera_frames_match_oracle(kl, name, case):
    _, sc = poisoned(name, case)
    check_frame(kl, name, case, sc, oracle_frame(sc))


@pytest.mark.parametrize("case", ENV_CASES)
@pytest.mark.parametrize("name", ["cornell", "soup150"])
def test_poisoned_environment_frames_match_oracle(kl, name, case):
    _, sc = poisoned(name, case)
    check_frame(kl, name, case, sc, oracle_frame(sc))


@pytest.mark.parametrize("case", PARTIAL_CASES)
@pytest.mark.parametrize("name", ["cornell", "soup150"])
def test_partly_poisoned_scenes_match_oracle_on_every_fast_path(kl, name, case):
    """Normals, materials and vertices poisoned in part: the frame differs from the clean one on at least 5 %
    of the pixels and equals it on at least 5 % (so both poisoned and clean paths are rendered; the ior cases
    must change nothing instead), REF and FAST equal the oracle, and every FAST path gives the same bits."""
    clean, sc = poisoned(name, case)
    want = oracle_frame(sc)
    changed = len(pixels_differing(want, oracle_frame(clean)))
    if case.startswith("ior"):
        # nothing reads a material's ior: glass passes rays straight through (Raytracing.cl:72-77), so no
        # value of it may change a single bit
        assert changed == 0
    else:
        assert -(-NPIX // 20) <= changed <= NPIX - -(-NPIX // 20), changed
    fast = check_frame(kl, name, case, sc, want)
    for path, options in other_fast_paths(sc).items():
        np.testing.assert_array_equal(render(kl, sc, "fast", **options), fast, err_msg=f"{name} {case}: {path}")


# ---- (c) worst-case stacks ----

# one-pass launches (pilot 0), so that the counters are those of one walk per ray
STACK_PATHS = [dict(bvh_width=2, stack_lds=0, pilot=0), dict(bvh_width=2, stack_lds=8, pilot=0),
               dict(bvh_width=4, stack_lds=0, pilot=0), dict(bvh_width=4, stack_lds=8, pilot=0),
               dict(bvh_width=2, walk_team=4, stack_lds=0, pilot=0), dict(bvh_width=2, walk_team=4, stack_lds=8, pilot=0)]


@pytest.mark.parametrize("name", ["soup2000", "caterpillar"])
def test_all_nan_camera_ends_every_ray_at_the_root(kl, name):
    """The all-NaN camera: every ray's slab distances are NaN on all three axes.  REF (the reference's
    tmax >= tmin) fetches the root and rejects it: one node and no triangle per ray, the oracle's counts.
    The FAST tree walks reject it in fast_init, before any fetch: no node, no triangle -- the NaN ray does
    NOT visit the whole tree (test_every_ray_visits_the_whole_caterpillar reaches the full visit)."""
    _, sc = poisoned(name, "cam_pos_nan_all")
    want, oc = oracle_frame(sc, counts=True)
    rc, _ = count(kl, sc, "ref")
    assert oc["nodes"] == oc["rays"] and oc["tris"] == 0
    assert (rc["rays"], rc["node_fetches"], rc["tri_tests"]) == (oc["rays"], oc["nodes"], 0)
    for options in STACK_PATHS:
        np.testing.assert_array_equal(render(kl, sc, "fast", **options), want, err_msg=str(options))
        fc, _ = count(kl, sc, "fast", fixed_point=0, **options)
        assert fc["rays"] == oc["rays"], options
        assert (fc["node_fetches"], fc["tri_tests"], fc["stack_drops"]) == (0, 0, 0), options


def test_every_ray_visits_the_whole_caterpillar(kl):
    """A finite ray that passes every box and hits nothing: from (1.4, -3.5, 1.4) along +y (a 0.02 rad field
    of view: x and z stay within 1.4 +- 0.07 up to the last triangle), inside every box of the caterpillar in
    x and z, past the triangles' apex side (at z = 1.4 a triangle spans |x| <= 0.05).  Both children of every
    node are hit and nothing culls, so the BVH2 walk holds one entry per internal node of the chain when it
    reaches the bottom: 39 = depth, the computed bound (20 in LDS and 19 in the overflow buffer, or 8 and 31),
    and the 4-wide walk holds its bound wdepth.  Every ray fetches every internal node once and tests every
    triangle once, on every walk."""
    sc = _ns(scene("caterpillar"), cam=np.array([1.4, -3.5, 1.4, 0, 0, 0, 32, 32, 1, 0.02], np.float32))
    leaf = sc.bvh.reshape(-1, 9)[:, 2:8]
    rays = np.array([O.camera_ray(sc.cam, i) for i in range(NPIX)])
    assert np.isfinite(rays).all() and NR.slab_pass(leaf[:, [0, 3, 1, 4, 2, 5]], rays).all()
    want, oc = oracle_frame(sc, counts=True)
    assert oc["dropped"] > 0 and oc["env"] == NPIX * SPP       # the reference's 20-slot stack overflows; all escape
    host = _native.scene_check(sc.V_p, sc.V_n, sc.faceData, sc.materialData, sc.bvh, layout=_native.RT_BVH_REFERENCE)
    assert (host["nodes"], host["depth"], host["tris"]) == (39, 39, 40) and host["wdepth"] > 11
    rc, _ = count(kl, sc, "ref")
    assert (rc["node_fetches"], rc["tri_tests"], rc["stack_drops"]) == (oc["nodes"], oc["tris"], oc["dropped"])
    for options in STACK_PATHS:
        np.testing.assert_array_equal(render(kl, sc, "fast", **options), want, err_msg=str(options))
        fc, info = count(kl, sc, "fast", fixed_point=0, **options)
        assert info["depth"] == 39 and fc["rays"] == oc["rays"], options
        nodes = host["wnodes"] if options["bvh_width"] == 4 else host["nodes"]
        assert fc["node_fetches"] == nodes * fc["rays"], (options, fc)
        assert fc["tri_tests"] == host["tris"] * fc["rays"], (options, fc)


def test_small_deep_tree_walk_equals_brute_force(kl):
    """The caterpillar from its usual camera, where hits matter: 40 triangles are few enough for the kernels
    that stage the scene in LDS, but its 39-level tree is deeper than any LDS stack, and those kernels have no
    spill path (an entry past stack_lds landed in the staged node array).  Such a scene walks global memory
    with the overflow buffer; every walk gives the brute-force frame, which tests all 40 triangles."""
    sc = scene("caterpillar")
    brute = render(kl, sc, "fast", brute_max=64)
    assert len(pixels_differing(brute, oracle_frame(sc))) > NPIX // 20     # the reference's stack drops the nearest
    for options in STACK_PATHS + [dict(step=2), dict(resume_min=0)]:
        np.testing.assert_array_equal(render(kl, sc, "fast", **options), brute, err_msg=str(options))
    # speculative trails (rt_spec.hip, with spill code): 16 samples, 14 of them left to the trails
    brute16 = render(kl, sc, "fast", spp=16, brute_max=64)
    for trails in (2, 4, 8):
        np.testing.assert_array_equal(render(kl, sc, "fast", spp=16, pilot=2, spec=trails, bvh_width=2), brute16,
                                      err_msg=f"trails {trails}")
    # the same with a tree that is only deeper than a reduced LDS stack
    sc = scene("soup150")
    want = render(kl, sc, "fast")
    np.testing.assert_array_equal(want, oracle_frame(sc))
    for options in (dict(stack_lds=8), dict(stack_lds=8, bvh_width=2, walk_team=2), dict(stack_lds=8, step=2),
                    dict(stack_lds=8, resume_min=0)):
        np.testing.assert_array_equal(render(kl, sc, "fast", **options), want, err_msg=str(options))


# ---- (d) schedules ----

# name: options.  Which kernel each reaches on soup150 depends on `base` below (staged in LDS or global memory).
SCHEDULES = {"fixed_point off": dict(fixed_point=0), "fixed_point on": dict(fixed_point=1),
             "sun_cache off": dict(sun_cache=0), "sun_cache on": dict(sun_cache=1),
             "two-pass pilot 2": dict(pilot=2, spec=0), "one pass, 2 sample slices": dict(pilot=0, slices=2),
             "plain walk (resume_min 0: render_kernel)": dict(resume_min=0),
             "resumable walk, shade when all 64 lanes are free": dict(resume_min=64),
             "item steps": dict(step=1), "descend-until-leaf rounds": dict(step=2)}


def test_schedules_render_the_zero_normal_scene_identically(kl):
    """soup150 with every third normal zero (NaN bounce directions; its materials include glass): every
    schedule and shortcut of the shading loop gives the one-shot frame, bit for bit.

    Each schedule runs twice.  With the default stack soup150 is staged in LDS: render_resume_kernel<SMEM>
    (render_kernel<SMEM> for resume_min 0), BVH2.  With stack_lds 8, below its depth of 10, it walks global
    memory with the overflow buffer: render_resume_kernel<OVF> with pipelined item steps (fast_step_pipe,
    top_levels; fast_round for step 2; render_kernel<OVF> for resume_min 0) -- the kernels of larger scenes.
    The speculative trails exist only for that second kind (spec_walk): they run at 16 samples, a 2-sample
    pilot leaving 14 to 2, 4 and 8 trails, so every trail has samples and meets NaN bounce directions."""
    _, sc = poisoned("soup150", "vn_zero_every_3rd")
    assert _native.scene_check(sc.V_p, sc.V_n, sc.faceData, sc.materialData, sc.bvh)["depth"] == 10
    want = oracle_frame(sc)
    one = render(kl, sc, "fast")
    np.testing.assert_array_equal(one, want)
    for base in (dict(), dict(stack_lds=8, bvh_width=2)):
        for name, options in SCHEDULES.items():
            np.testing.assert_array_equal(render(kl, sc, "fast", **base, **options), one, err_msg=f"{name} {base}")
    # speculative trails forced (rt_spec.hip spec_kernel continues pass 2), in global memory
    want16 = oracle_frame(sc, spp=16)
    np.testing.assert_array_equal(render(kl, sc, "fast", spp=16), want16)
    for trails in (2, 4, 8):
        got = render(kl, sc, "fast", spp=16, pilot=2, spec=trails, bvh_width=2, stack_lds=8)
        np.testing.assert_array_equal(got, want16, err_msg=f"trails {trails}")
    # an unlit sun: the shadow-ray shortcut on and off
    dark = _ns(sc, env=np.array([*sc.env[:3], 0.0, sc.env[4]], np.float32))
    want_dark = oracle_frame(dark)
    for base in (dict(), dict(stack_lds=8, bvh_width=2)):
        for skip in (0, 1):
            np.testing.assert_array_equal(render(kl, dark, "fast", sun_skip=skip, **base), want_dark,
                                          err_msg=f"sun_skip {skip} {base}")
    # progressive accumulation: 2 + 2 samples, staged and in global memory
    for base in (dict(), dict(stack_lds=8, bvh_width=2)):
        render(kl, sc, "fast")
        kl.set_traversal("fast")
        ctx = kl.native
        with options_set(kl, sc, base):
            ctx.accum_begin(sc.cam, sc.env, NPIX, MB)
            try:
                two = ctx.accum_add(2).copy()
                four = ctx.accum_add(2).copy()
            finally:
                ctx.accum_end()
        np.testing.assert_array_equal(two, oracle_frame(sc, spp=2), err_msg=str(base))
        np.testing.assert_array_equal(four, one, err_msg=str(base))


def test_wide_walk_camera_check_with_nan_components(kl):
    """choose_kernel picks the origin-folded dequantisation of the 4-wide walk when every camera coordinate is
    within DevScene::wdq_omax.  The check must be false for a NaN coordinate in any position (std::max drops
    a NaN second operand, so a maximum over the three would keep only a NaN in cam[0]).  soup2000 is too large
    to stage in LDS, so bvh_width 4 is the 4-wide walk; with wdq on and off the frame is the oracle's."""
    base = scene("soup2000")
    for axis in range(3):
        cam = base.cam.copy()
        cam[axis] = NAN
        sc = _ns(base, cam=cam)
        want = oracle_frame(sc)
        for wdq in (1, 0):
            for lds in (0, 8):
                got = render(kl, sc, "fast", bvh_width=4, wdq=wdq, stack_lds=lds)
                np.testing.assert_array_equal(got, want, err_msg=f"cam[{axis}] NaN, wdq {wdq}, stack_lds {lds}")
    # the finite camera, where the rays do walk: both dequantisations give the oracle's frame
    want = oracle_frame(base)
    for wdq in (1, 0):
        np.testing.assert_array_equal(render(kl, base, "fast", bvh_width=4, wdq=wdq), want, err_msg=f"wdq {wdq}")
