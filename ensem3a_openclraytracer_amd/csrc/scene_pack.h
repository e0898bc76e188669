// Host-side scene preparation (no HIP): validates the reference's flat scene arrays and packs
// them into the device layouts of rt_internal.h.  rt_set_scene (rt_api.hip) uploads the result;
// rt_scene_check (include/rt_scene.h) runs it alone, without a GPU.  Not part of the public
// boundary.  Host-only, so it builds with -fsanitize=address,undefined (oracle/Makefile asan).
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "rt_layout.h"

namespace rt {

// Host copy of the packed scene (kept to upload on every device).
struct HostScene {
    std::vector<float> nodes;      // 16 floats per internal node
    std::vector<float> wnodes;     // wide layout: 16 floats per 4-wide node (DevScene::wnodes)
    std::vector<float> wleaves;    // wide layout: 16 floats per leaf, in reference DFS rank order
    int32_t nwnodes = 0, wroot_ref = 0, wdepth = 1;
    float wdq_omax = 0.0f;   // the 4-wide layout's dequantisation gap covers ray origins up to this (0: no gap)
    std::vector<float> bvh9;
    std::vector<float> tri_geo;    // 12 floats per triangle
    std::vector<float> tri_fast;   // tri_geo's records in FAST leaf order (DevScene::tri_fast)
    std::vector<float> tri_shade;  // 4 floats per triangle
    std::vector<float> mat;
    std::vector<float> brute;      // 16 floats per triangle, small scenes only (rt_internal.h DevScene::brute)
    std::vector<float> brute_box;  // 8 floats per triangle, padded to whole groups (DevScene::brute_box)
    int32_t nbrute = 0;
    int32_t nbox = 0;              // distinct leaf boxes in brute_box (records with bit-identical boxes share one)
    // the clustered form of brute_box (DevScene::brute_cbox / brute_crow; ncluster = 0: not clustered)
    std::vector<float> brute_cbox; // 8 floats per slot: the single slots padded to whole groups, then kClusterSlots per cluster
    std::vector<float> brute_crow; // 8 floats per cluster: union lo.x hi.x lo.y hi.y lo.z hi.z | first slot, box count
    int32_t ncluster = 0, nsingle = 0;   // clusters; single (real) slots at the head of brute_cbox
    // the shell among the single slots (scene_pack.cpp build_shell, option "brute_shell"; nshell = 0: none):
    // kShellRecF floats -- the shell box lo.x hi.x lo.y hi.y | lo.z hi.z, nrest, nshell | nquad << 8 (int bits) | the two
    // records of the faces -x +x | -y +y | -z +z (int bits; an absent face -1 -1) -- then the nrest singles that
    // are no face, 8 floats per slot in brute_cbox order, padded to whole groups
    // -- | kShellRows rows of 8 floats (rt_layout.h: each face's line, packed records and flags, option
    // "brute_quad"; scene_pack.cpp quad_split)
    std::vector<float> brute_shell;
    int32_t nshell = 0, nrest = 0;       // faces of the shell; single slots outside it
    int32_t nquad = 0;                   // faces the packer split (option "brute_quad")
    // option "brute_near" (scene_pack.cpp near_safe): 1 for each of the nbox boxes of brute_box that
    // is near-safe -- a ray that passes it closer than rt::kNearFloor cannot hit its records -- and the floor of the
    // shell's face tests: rt::kNearFloor when the shell's every face is such a box, else 0
    std::vector<uint8_t> brute_near;
    float shell_floor = 0.0f;
    uint64_t shell_mask = 0;   // bit g: box g of brute_box (g < 64) is a face of the shell (DevScene::near_mask_lo / _hi)
    int32_t nnodes = 0, root_ref = 0, ntri = 0, nmat = 0, nbvh9 = 0, depth = 1;
    float root_box[6] = {0, 0, 0, 0, 0, 0};
    bool fast_ok = false;
    bool colors_finite = true;     // every material colour finite (FrameParams::sun_skip)
    bool has_glass = false;        // some material has type 3 (FrameParams::sun_any)
    bool diffuse_only = true;      // every material has type 0 or 1 (materials_diffuse_only; the lean brute-force kernels)
};

// The census behind HostScene::diffuse_only: every one of the nmat6 / 6 material rows (6 floats each, the type first)
// has type 0 (emissive) or 1 (diffuse) as the kernels read it, (int)type.  True for an empty table.
bool materials_diffuse_only(const float* mat, int64_t nmat6);


// Validate and pack (KernelLauncher.py:38-72's buffers, FileManager.py:276-282's faceData,
// BVH.py:174-191's export).  Returns RT_OK, or an RT_ERR_* code with `msg` set.  `why` receives the
// reason when the FAST layouts are unavailable (hs.fast_ok false; the REF traversal then serves).
int scene_prepare(HostScene& hs, const float* vp, int64_t nvp, const float* vn, int64_t nvn, const int32_t* face,
                  int64_t nface, const float* mat, int64_t nmat, const float* bvh9, int64_t nbvh, int layout,
                  int brute_max, int cluster, int shell, int quad, std::string& msg, std::string& why);

// pack_fast + the limits of the FAST kernels; sets hs.fast_ok (an option change repacks with it).
// cluster, shell: options "brute_cluster", "brute_shell" (0 off, -1 auto, 1 force; include/rt_debug.h); quad: option
// "brute_quad" (0: no face of the shell is split, else auto).
void pack_checked(HostScene& hs, const float* bvh9, int64_t nb, int64_t ntri, int layout, int brute_max, int cluster,
                  int shell, int quad, std::string& why);

// Option "brute_direct" (0 off, else auto): the bit kShellDirect of the shell record's count word, set exactly when
// the option is on and the packed scene has a shell.  The callers of scene_prepare / pack_checked call it after
// every pack; true when the record carries the bit.
bool shell_direct(HostScene& hs, int direct);

}  // namespace rt
