// Layout constants shared by the host scene packer (scene_pack.cpp, no HIP) and the kernels
// (rt_internal.h).  Not part of the public boundary.
#pragma once
#include <cstddef>
#include <cstdint>

namespace rt {

// LDS entries of the FAST traversal stack per lane (int2 each); deeper entries spill to HBM.
constexpr int kStackLds = 20;
// ... and on the 4-wide walk, whose kernel runs 7 waves per SIMD (render_resume_kernel, kWideWaves):
// 11 entries (88 B per lane) leave the LDS room for them (C5 at 7 waves: 5,890 ms with 11 entries,
// 5,915 with 10)
constexpr int kStackLdsWide = 11;
#ifndef RT_WIDE_WAVES
#define RT_WIDE_WAVES 7   // variant builds (tools/variants.py) override it for the spill A/B
#endif
constexpr int kWideWaves = RT_WIDE_WAVES;   // waves per SIMD of the 4-wide walk (rt_kernels.hip)
constexpr int kNodeF4 = 4;             // float4 per FAST BVH2 node (DevScene::nodes)
constexpr int kMaxLanesPerCu = 2048;   // resident threads per CU (gfx950)
#ifndef RT_BOX_GROUP
#define RT_BOX_GROUP 4
#endif
constexpr int kBoxGroup = RT_BOX_GROUP;  // leaf boxes per scalar load group of the brute-force loop (DevScene::brute_box)
// Clustered brute force (DevScene::brute_cbox, option "brute_cluster"): a cluster holds up to kClusterSlots
// distinct leaf boxes in kClusterSlots slots (padded), so an item index splits into (owner, box) with a
// shift and a mask.  A subtree of m boxes whose union has the share p of the root's surface area becomes a
// cluster when its estimated cost 1 + kappa p kClusterSlots (one union test, then the passing rays'
// compacted (ray, box) items, padding slots included) is below kClusterGain m (m lock-step tests; 3/4: "clearly
// below").  kappa = the VALU instructions -- the kernel is bound by VALU issue, DESIGN.md 5.1 -- a wave issues
// per batch of 64 compacted items over those per lock-step box, counted in the built gfx950 kernel (DESIGN.md
// 5.2): 62 (owner-list and LDS table addressing, slab test, two ring writes) against 32 (22 slab + 10 queue).
constexpr int kClusterShift = 3;
constexpr int kClusterSlots = 1 << kClusterShift;
constexpr double kClusterKappa = 1.9;
constexpr double kClusterGain = 0.75;
// a cluster whose union more than kClusterLockNum / 8 of the wave's tracing lanes pass runs its slots
// lock-step: n passing lanes cost n kClusterSlots / nact item batches against kClusterSlots lock-step
// boxes, equal at n = nact / kappa = 0.53 nact
constexpr int kClusterLockNum = 4;
// The shell among a clustered scene's single slots (scene_pack.cpp build_shell, option "brute_shell"): its record
// is kShellRecF floats (5 float4 and the rows below), the remaining singles' slots follow it.  auto takes a shell from kShellMinFaces
// faces: the smallest count at which the shell piece issues fewer VALU + SALU instructions than as many single
// tests, counted in the built gfx950 kernel: n single tests are 23 n VALU; the shell piece is 18
// shared VALU (6 subtracts, 6 multiplies, 3 min / max pairs), up to 8 canonicalising v_max, 5 VALU per face (3
// for the second of a -z +z pair) and 12 SALU (a compare and a branch per face position) -- at most 48 against 46
// for two faces, at most 53 against 69 for three
// Behind those 5 float4 the record carries kShellRows rows of 2 float4, one per face position -x +x -y +y -z +z and
// a last one for "no face" (option "brute_quad", scene_pack.cpp quad_split): the face's line A.x A.y A.z gamma |
// its packed records first | second << 16 (both, the one on sigma >= 0, the one on sigma < 0; ~0u: none), flags
// (bit 0 split, bit 1 the first record is on the positive side).  A face that is not split has a zero line.  The
// record's face count carries the number of split faces above bit 8 (0: the rule is off).
constexpr int kShellRows = 7;
constexpr int kShellRowF4 = 5;                     // where the rows start in the record, in float4
constexpr int kShellRecF = 20 + 8 * kShellRows;
constexpr int kShellMinFaces = 3;
// ... and, above the split faces, the enable of the first record's in-place test (option "brute_direct",
// scene_pack.cpp shell_direct; rt_device.h trace_brute_compact's one queue step)
constexpr int32_t kShellDirect = 1 << 16;
// The one queue step's choice between a split wall's two records (option "brute_quad"; DESIGN.md 4.2 has the proof).
// A lane is sure of its side sigma~ = A . (o + T d) + gamma of the wall's diagonal, and queues that side's record
// alone, when the origin lies in the shell's box, kQuadGraze max|d| <= |d_a| for the wall's axis a, max|d| <=
// kQuadDirMax and |sigma~| >= kQuadBand.  The packer splits a wall only when kQuadBand is at least kQuadSafety
// times the wall's own error bound (the classifier's and Moller-Trumbore's on the dropped record, plus kQuadSlack
// for the packer's double arithmetic, scaled by the triangles' height ratio, at most kQuadRatio), its records cancel
// by at most kQuadKappa and every component lies within 2^+-kQuadExp.  Cornell's walls' bound is 2^-17.6: 8 times that
// is 2^6 below the band, which leaves 1 - 2^-7 of a wall's width outside it.  Not tuned to any frame time
constexpr float kQuadBand = 0x1p-8f;
constexpr float kQuadGraze = 0x1p-6f;
constexpr float kQuadDirMax = 2.0f;
constexpr double kQuadSafety = 8.0;
constexpr double kQuadSlack = 0x1p-20;
constexpr double kQuadRatio = 4.0;
constexpr double kQuadKappa = 4.0;
constexpr int kQuadExp = 24;
// The floor of the shell's face tests (option "brute_near", DevScene::near_floor; DESIGN.md 4.2 has the proof).  A
// ray that starts on a wall passes that wall's flat box at a plane distance t of 0 to a few 1e-7, and the wall's
// triangles then return k = t up to rounding, which the k > 0.0001f of the hit condition throws away.  A face test
// whose lower clamp is this floor instead of 0 drops such passes before they are queued.  It stays 2^-12 below the
// 0.0001f of the hit condition; for a box the packer found near-safe (scene_pack.cpp near_safe: flat on one axis,
// its records in that plane, cancellation factor kappa <= kNearKappa, components within 2^+-kNearExp) k exceeds t
// by less than 2^-13.9 of it, so every dropped pair is one Moller-Trumbore rejects.  0.0f: today's test
constexpr float kNearFloor = 0.0001f * (1.0f - 0x1p-12f);
constexpr double kNearKappa = 256.0;   // (|e1b e2c| + |e1c e2b|) / |e1b e2c - e1c e2b| of a near-safe record, at most
constexpr int kNearExp = 40;           // its non-zero components, and the box's bounds, lie in [2^-40, 2^40]
#ifndef RT_BRUTE_MAX_DEFAULT
#define RT_BRUTE_MAX_DEFAULT 64   // FAST tests every triangle of scenes up to this size (rt_set_option "brute_max")
#endif
constexpr int kMatF = 8;               // floats per device material row (DevScene::mat)
// FAST tree walk over the 4-wide layout when the BVH2 node array exceeds this (option "bvh_width"
// 0 = auto): trees that do not fit the L2, where the walk is bound by the latency of dependent
// misses and half as many node fetches pay; smaller trees are bound by the item step's VALU.
constexpr size_t kWideMinBytes = 16u << 20;

// Per-launch scratch block (the `work` argument of launch_render): pixel hand-out counters of the
// kGroups block groups (blockIdx.x % kGroups: the blocks one XCD runs under round-robin dispatch),
// kCounterStride bytes apart, then the per-launch constants at kConstOffset.
constexpr int kGroups = 8;
constexpr int kCounterStride = 64;
constexpr int kTeamOffset = 512;    // pilot launches: pixels left after pass 1 (uint32), then the pass-2 team size (int32)
constexpr int kConstOffset = 1024;
constexpr int kWorkBytes = 2048;
// Tile pixels are dealt to the groups in chunks of kChunk consecutive pixels (chunk c to group
// c % kGroups), so each 128-byte line of the frame is written by the blocks of one XCD only.
constexpr int kChunkShift = 10;

}  // namespace rt
