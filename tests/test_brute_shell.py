"""The shell among a clustered scene's single slots (rt_debug_brute_shell, option "brute_shell"; scene_pack.cpp
build_shell, rt_device.h trace_brute_compact), on the host alone: which box and which slots the packer takes, that
the shell's faces and the remaining table partition the single slots, and -- in numpy -- that a face's test from the
box's six shared plane distances gives slab()'s own tmin and tmax on the face's box, bit for bit."""
import types

import numpy as np
import pytest

from ensem3a_openclraytracer_amd import _native
from tests import nonfinite_rays as NR
from tests.test_brute_clusters import GPU_SOUPS
from tests.test_malformed_inputs import BRUTE_SCENES, _brute_scene

MIN_FACES = 3        # rt_layout.h kShellMinFaces (auto); force takes a shell from the 2 faces that define one
FACES = ("-x", "+x", "-y", "+y", "-z", "+z")
UNIT = (-1.0, 1.0, -1.0, 1.0, -1.0, 1.0)
ONE_ULP_SHORT = float(np.nextafter(np.float32(1.0), np.float32(0.0)))


def wall_box(room, f, short=None):
    """The box of face f (0..5: -x +x -y +y -z +z) of room (lo.x hi.x lo.y hi.y lo.z hi.z); short = (k, v): bound k
    of the wall is v instead of the room's."""
    b = np.array(room, np.float32)
    b[2 * (f // 2)] = b[2 * (f // 2) + 1] = room[f]
    if short is not None:
        b[short[0]] = short[1]
    return b


def room_scene(walls, blocks=2, seed=0):
    """A soup built like tests/test_gpu_parity.py _random_scene: `walls` (boxes from wall_box) as quads of two
    triangles, whose leaf boxes are the wall's box, bit for bit, and share a slot; then `blocks` tight groups of 8
    small triangles near (0.45, 0.3, -0.6) and (-0.5, -0.2, -0.55), which the packer clusters (their unions are a
    small share of the scene's surface) while the walls stay single slots."""
    from ensem3a_openclraytracer_amd import bvh as B
    rng = np.random.default_rng(500 + seed)
    tris, mats = [], []
    for w in walls:
        w = np.asarray(w, np.float32)
        a = int(np.argmax(w[0::2] == w[1::2]))
        u, v = [k for k in range(3) if k != a]
        c = np.zeros((4, 3), np.float32)
        c[:, a] = w[2 * a]
        c[:, u] = [w[2 * u], w[2 * u + 1], w[2 * u + 1], w[2 * u]]
        c[:, v] = [w[2 * v], w[2 * v], w[2 * v + 1], w[2 * v + 1]]
        tris += [c[[0, 1, 2]], c[[0, 2, 3]]]
        mats += [len(mats) // 2 % 2 * 4] * 2                 # diffuse, two colours
    for k, centre in enumerate(([0.45, 0.3, -0.6], [-0.5, -0.2, -0.55])[:blocks]):
        for j in range(8):
            p = np.asarray(centre) + rng.uniform(-0.06, 0.06, 3)
            tris.append((p + rng.normal(0.0, 0.03, (3, 3))).astype(np.float32))
            mats.append(3 if j == 0 else 1 + (j + k) % 2)    # an emitter, glossy and glass
    tri = np.asarray(tris, np.float32)
    n = len(tri)
    vp = tri.reshape(-1, 3)
    e1, e2 = tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
    nrm = np.cross(e1, e2)
    nrm = (nrm / np.maximum(np.linalg.norm(nrm, axis=1, keepdims=True), 1e-20)).astype(np.float32)
    mat = np.array([[1, 0.8, 0.7, 0.6, 0.0, 1.0], [2, 0.9, 0.9, 0.9, 0.25, 1.0], [3, 0.95, 1.0, 1.0, 0.0, 1.5],
                    [0, 1.0, 1.0, 1.0, 3.0, 1.0], [1, 0.2, 0.5, 0.9, 0.0, 1.0]], np.float32)
    face = np.zeros((n, 10), np.int32)
    face[:, 0] = mats
    face[:, 4:7] = np.arange(n)[:, None]
    face[:, 7:10] = np.arange(3 * n).reshape(n, 3)
    fd = face.ravel()
    return types.SimpleNamespace(V_p=vp.ravel(), V_n=nrm.ravel(), V_uv=np.zeros(2, np.float32), faceData=fd,
                                 materialData=mat.ravel(), lightData=np.zeros(0, np.float32), BVH=B.BVH(fd, vp.ravel()))


def six_face_room():
    return room_scene([wall_box(UNIT, f) for f in range(6)])


def one_ulp_room():
    """The +x wall ends one ulp short of the room on y: a single, not a face."""
    return room_scene([wall_box(UNIT, f, (3, ONE_ULP_SHORT) if f == 1 else None) for f in range(6)])


def _args(sc):
    return sc.V_p, sc.V_n, sc.faceData, sc.materialData, sc.BVH.exportArray


def _singles(sc, cluster=-1):
    slots, rows, nsingle = _native.brute_clusters(*_args(sc), cluster)
    return slots[:nsingle], len(rows)


def _ids(slots):
    return slots[:, 6:8].copy().view(np.int32)


def _faces_of(singles, room):
    """The face definition restated: slot -> face position of `room`, every equality bitwise."""
    room = np.asarray(room, np.float32)
    out = {}
    for s, b in enumerate(singles[:, :6]):
        for f in range(6):
            if b.tobytes() == wall_box(room, f).tobytes() and f not in out.values():
                out[s] = f
    return out


def _check_shell(sc, sh, room, want_faces, cluster=-1):
    """sh is the shell of `room` with the walls at the positions want_faces, and partitions the single slots."""
    singles, _ = _singles(sc, cluster)
    assert sh is not None
    assert sh["box"].tobytes() == np.asarray(room, np.float32).tobytes()
    fs = _faces_of(singles, room)
    assert sorted(fs.values()) == sorted(want_faces)
    ids = _ids(singles)
    for f in range(6):
        if f in want_faces:
            s = [k for k, v in fs.items() if v == f][0]
            assert sh["faces"][f].tolist() == ids[s].tolist(), FACES[f]
        else:
            assert sh["faces"][f].tolist() == [-1, -1], FACES[f]
    assert sh["nfaces"] == len(want_faces) and sh["nrest"] == len(singles) - len(want_faces)
    rest = [s for s in range(len(singles)) if s not in fs]
    assert sh["rest"][:sh["nrest"]].tobytes() == singles[rest].tobytes()        # the others, in their order
    return fs


def test_cornell_shell_is_the_room_with_five_walls():
    sc = _brute_scene("cornell")
    sh = _native.brute_shell(*_args(sc))
    fs = _check_shell(sc, sh, UNIT, [0, 1, 3, 4, 5])                              # open towards the camera (-y)
    assert sorted(fs) == [0, 1, 2, 4, 5]                                          # slot 3 is the light
    singles, ncl = _singles(sc)
    assert ncl == 2 and sh["nrest"] == 1 and sh["rest"][0].tobytes() == singles[3].tobytes()
    assert _native.brute_shell(*_args(sc), -1, 1)["faces"].tolist() == sh["faces"].tolist()   # force: the same
    assert _native.brute_shell(*_args(sc), -1, 0) is None


def test_six_face_room():
    sc = six_face_room()
    singles, ncl = _singles(sc)
    assert ncl == 2 and len(singles) == 6
    sh = _native.brute_shell(*_args(sc))
    _check_shell(sc, sh, UNIT, range(6))
    assert sh["nrest"] == 0 and len(sh["rest"]) == 0


def test_a_wall_one_ulp_short_is_a_single():
    sc = one_ulp_room()
    sh = _native.brute_shell(*_args(sc))
    _check_shell(sc, sh, UNIT, [0, 2, 3, 4, 5])
    short = wall_box(UNIT, 1, (3, ONE_ULP_SHORT))
    assert sh["nrest"] == 1 and sh["rest"][0, :6].tobytes() == short.tobytes()


OTHER = (1.5, 3.5, -1.25, 1.0, -1.0, 1.5)


def _two_rooms(nbig, nother, other_first=False):
    big = [wall_box(UNIT, f) for f in range(nbig)]
    small = [wall_box(OTHER, f) for f in range(6 - nother, 6)]
    return room_scene(small + big if other_first else big + small)


@pytest.mark.parametrize("other_first", (False, True))
def test_two_rooms_the_larger_face_count_wins(other_first):
    sc = _two_rooms(5, 4, other_first)
    _check_shell(sc, _native.brute_shell(*_args(sc)), UNIT, range(5))
    sc = _two_rooms(3, 5, other_first)
    _check_shell(sc, _native.brute_shell(*_args(sc)), OTHER, range(1, 6))


@pytest.mark.parametrize("other_first", (False, True))
def test_two_rooms_tie_goes_to_the_lowest_first_slot(other_first):
    sc = _two_rooms(4, 4, other_first)
    singles, _ = _singles(sc)
    a, b = _faces_of(singles, UNIT), _faces_of(singles, OTHER)
    assert len(a) == 4 and len(b) == 4
    room, fs = (UNIT, a) if min(a) < min(b) else (OTHER, b)
    _check_shell(sc, _native.brute_shell(*_args(sc)), room, sorted(fs.values()))
    # the same scene twice: the same table
    assert _native.brute_shell(*_args(sc))["faces"].tolist() == _native.brute_shell(*_args(sc))["faces"].tolist()


def test_below_the_minimum_face_count_there_is_no_shell():
    sc = room_scene([wall_box(UNIT, f) for f in range(MIN_FACES - 1)])
    singles, ncl = _singles(sc)
    assert ncl > 0 and len(_faces_of(singles, UNIT)) == MIN_FACES - 1
    assert _native.brute_shell(*_args(sc)) is None
    if MIN_FACES > 2:                                        # force: from the two faces that define a shell
        _check_shell(sc, _native.brute_shell(*_args(sc), -1, 1), UNIT, range(MIN_FACES - 1))
    sc = room_scene([wall_box(UNIT, f) for f in range(MIN_FACES)])
    _check_shell(sc, _native.brute_shell(*_args(sc)), UNIT, range(MIN_FACES))


def test_a_scene_that_is_not_clustered_has_no_shell():
    sc = room_scene([wall_box(UNIT, f) for f in range(6)], blocks=0)    # the walls alone: nothing to cluster
    assert _singles(sc)[1] == 0
    for mode in (-1, 1):
        assert _native.brute_shell(*_args(sc), -1, mode) is None
    sc = six_face_room()
    assert _native.brute_shell(*_args(sc), 0, 1) is None                 # option "brute_cluster" off
    with pytest.raises(_native.NativeError):
        _native.brute_shell(*_args(sc), -1, 2)


ROOMS = {"six": six_face_room, "ulp": one_ulp_room, "two": lambda: _two_rooms(4, 4)}


@pytest.mark.parametrize("shell", (-1, 1))
@pytest.mark.parametrize("cluster", (-1, 1))
@pytest.mark.parametrize("which", BRUTE_SCENES + GPU_SOUPS + list(ROOMS), ids=str)
def test_faces_and_rest_partition_the_single_slots(which, cluster, shell):
    sc = ROOMS[which]() if which in ROOMS else _brute_scene(which)
    singles, ncl = _singles(sc, cluster)
    sh = _native.brute_shell(*_args(sc), cluster, shell)
    if sh is None:
        return
    assert ncl > 0 and sh["nfaces"] >= (MIN_FACES if shell < 0 else 2)
    nbrute = sc.faceData.size // 10
    ids, got = _ids(singles), []
    for f in range(6):
        qa, qb = sh["faces"][f]
        if qa < 0:
            assert qb == -1
            continue
        s = [k for k in range(len(singles)) if ids[k].tolist() == [qa, qb]]
        assert len(s) == 1 and 0 <= qa < nbrute and -1 <= qb < nbrute
        assert singles[s[0], :6].tobytes() == wall_box(sh["box"], f).tobytes()   # a face, at its position
        got.append(s[0])
    assert len(got) == sh["nfaces"] and len(set(got)) == len(got)
    rest = sh["rest"]
    assert sh["nrest"] == len(singles) - len(got) and len(rest) == -(-sh["nrest"] // 4) * 4
    assert rest[:sh["nrest"]].tobytes() == singles[[s for s in range(len(singles)) if s not in got]].tobytes()
    # padding: the point at 1e30 listing record 0 alone -- never a face: the shell box is finite with lo < hi
    pad = rest[sh["nrest"]:]
    assert (pad[:, :6] == np.float32(1e30)).all() and (_ids(pad) == [0, -1]).all()
    assert np.isfinite(sh["box"]).all() and (sh["box"][0::2] < sh["box"][1::2]).all()


def _slab(box, rays):
    """rt_device.h slab() in float32 numpy: (tmin, tmax) of rays (R, 6: dir, origin) on one box."""
    with np.errstate(all="ignore"):
        inv = np.float32(1.0) / rays[:, 0:3]
        t0, t1 = (box[0::2] - rays[:, 3:6]) * inv, (box[1::2] - rays[:, 3:6]) * inv
        near, far = np.fmin(t0, t1), np.fmax(t0, t1)
        return (np.fmax(np.fmax(near[:, 0], near[:, 1]), near[:, 2]),
                np.fmin(np.fmin(far[:, 0], far[:, 1]), far[:, 2]))


def _shell_faces(room, rays):
    """The shell piece of trace_brute_compact in float32 numpy: the six plane distances and each axis's min / max
    once, then per face slab()'s two nests with the flat axis's one distance for both its min and its max."""
    with np.errstate(all="ignore"):
        inv = np.float32(1.0) / rays[:, 0:3]
        t = np.stack([(room[k] - rays[:, 3 + k // 2]) * inv[:, k // 2] for k in range(6)], axis=1)   # (R, 6)
        mn = [np.fmin(t[:, 2 * a], t[:, 2 * a + 1]) for a in range(3)]
        mx = [np.fmax(t[:, 2 * a], t[:, 2 * a + 1]) for a in range(3)]
        out = []
        for f in range(6):
            lo = [t[:, f] if a == f // 2 else mn[a] for a in range(3)]
            hi = [t[:, f] if a == f // 2 else mx[a] for a in range(3)]
            out.append((np.fmax(np.fmax(lo[0], lo[1]), lo[2]), np.fmin(np.fmin(hi[0], hi[1]), hi[2])))
        return out


@pytest.mark.parametrize("room", (UNIT, OTHER, (-1.0, 1.0, -0.0, 0.0078125, -3e38, 1e-40)), ids=str)
def test_face_test_equals_slab_bit_for_bit(room):
    room = np.asarray(room, np.float32)
    rng = np.random.default_rng(11)
    n = 200_000
    d = NR.unit_dirs(rng, n)
    o = rng.uniform(-3.0, 3.0, (n, 3)).astype(np.float32)
    k = np.arange(n)
    d[k % 7 == 0, 0] = np.float32(0.0)                       # zero and -0 direction components
    d[k % 11 == 0, 1] = np.float32(-0.0)
    d[k % 13 == 0, 2] = np.float32(0.0)
    for a in range(3):                                       # origins on a plane of the room
        o[k % 5 == a, a] = room[2 * a + (a % 2)]
        o[k % 17 == a, a] = room[2 * a + 1 - (a % 2)]
    d[k % 101 == 0, 0] = np.float32(np.nan)                  # NaN and infinite components
    o[k % 103 == 0, 1] = np.float32(np.nan)
    d[k % 107 == 0, 2] = np.float32(np.inf)
    o[k % 109 == 0, 0] = np.float32(-np.inf)
    d[k % 113 == 0, 1] = np.float32(1e-40)                   # a denormal
    rays = [np.concatenate([d, o], axis=1)]
    leaf = np.stack([np.concatenate([wall_box(room, f)[0::2], wall_box(room, f)[1::2]]) for f in range(6)])
    with np.errstate(all="ignore"):                          # (the third room's bounds overflow a centre)
        rays += list(NR.ray_classes([0.0, -3.5, 0.0], leaf, seed=3).values())
    rays = np.concatenate(rays).astype(np.float32)
    got = _shell_faces(room, rays)
    for f in range(6):
        tn, tx = _slab(wall_box(room, f), rays)
        assert got[f][0].view(np.uint32).tobytes() == tn.view(np.uint32).tobytes(), FACES[f]
        assert got[f][1].view(np.uint32).tobytes() == tx.view(np.uint32).tobytes(), FACES[f]
        same = NR.slab_pass(wall_box(room, f), rays)[:, 0]
        with np.errstate(all="ignore"):
            assert ((np.fmax(got[f][0], np.float32(0)) <= np.fmin(got[f][1], NR.CULL)) == same).all()
