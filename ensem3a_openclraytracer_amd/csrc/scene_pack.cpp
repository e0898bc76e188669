// Host-side scene preparation (scene_pack.h): the reference's flat arrays -> the device layouts.
// Host-only C++ (no HIP), so the sanitizer build (oracle/Makefile asan) covers it.
#include "scene_pack.h"

#include <algorithm>
#include <array>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <atomic>
#include <functional>
#include <map>
#include <mutex>
#include <new>
#include <stdexcept>
#include <string>
#include <system_error>
#include <thread>
#include <vector>

#include "../../include/rt_api.h"
#include "../../include/rt_debug.h"
#include "../../include/rt_scene.h"
#include "bvh_sah.h"
#include "rtm.h"

using rt::HostScene;

namespace {

inline int32_t as_i32(float f) {
    int32_t i;
    std::memcpy(&i, &f, 4);
    return i;
}
inline float as_f32(int32_t i) {
    float f;
    std::memcpy(&f, &i, 4);
    return f;
}

// Reference index stored as float -> int, like (int)BVH[...] in MathLib.cl.
// Returns false for values the kernel could not use safely.
inline bool fidx(float v, int64_t limit, int32_t* out) {
    if (!(v == v) || v < -1.0f || v >= (float)limit + 1.0f) return false;
    const int32_t i = (int32_t)v;
    if (i < -1 || i >= limit) return false;
    *out = i;
    return true;
}

// p + q * s in fp32 (q * s is exact: s is a power of two): a quantised box bound, exactly as the
// kernels dequantise it (rt_kernels.hip wide_step; this file is built with -ffp-contract=off).
inline float deq(float p, uint32_t q, float s) { return p + (float)q * s; }

// A padding slot of DevScene::brute_box (8 floats): a point at 1e30, which no finite ray near the
// scene reaches within k < 1000, listing record 0 alone.  The product build of the brute-force loop
// queues whatever a passing slot lists, and the slab test does pass here for some rays: fminf / fmaxf
// drop NaN operands, so a ray with a NaN origin or direction passes every box, and so does a ray from
// (1e30, 1e30, 1e30) (every slab distance 0).  Such a pass then tests record 0 once more for its owner,
// which cannot change the owner's minimum (distance, rank) key.  Record 0 always exists: the record
// array holds at least one (zero) record.
inline void pad_box(float* b) {
    for (int k = 0; k < 6; ++k) b[k] = 1e30f;
    b[6] = as_f32(0);
    b[7] = as_f32(-1);
}


// f(begin, end) over [0, n) in chunks of `grain`, on up to 16 host threads (the caller's included)
template <class F>
void parallel_for(int64_t n, int64_t grain, F f) {
    const int64_t chunks = (n + grain - 1) / grain;
    const int nt = (int)std::min<int64_t>(chunks, std::max(1u, std::min(16u, std::thread::hardware_concurrency())));
    if (nt <= 1) {
        if (n > 0) f(0, n);
        return;
    }
    std::atomic<int64_t> next{0};
    auto run = [&]() {
        for (int64_t k; (k = next.fetch_add(1)) < chunks;) f(k * grain, std::min(n, (k + 1) * grain));
    };
    std::vector<std::thread> pool;
    for (int t = 1; t < nt; ++t) {
        try {
            pool.emplace_back(run);
        } catch (const std::system_error&) {   // no more threads: the ones started (and this one) do the rest
            break;
        }
    }
    run();
    for (auto& t : pool) t.join();
}

int fail(std::string& msg, int code, const char* fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    msg = buf;
    return code;
}

}  // namespace

// Per-axis quantisation of up to 4 child boxes against their union's lower corner p: a scale
// 2^e and byte bounds whose dequantised box contains each child's exact box.  Returns the
// biased exponent byte (scale = as_float(e << 23)), or -1 when no exponent up to 2^100 gives
// containing bounds (non-finite bounds, or an extent beyond 255 * 2^100): the caller must then not
// use the quantised layout (a dequantised box that is not a superset could cull a hit subtree).
extern "C" int rt_debug_quantise_axis(float p, const float* lo, const float* hi, int n, float gap, uint8_t* qlo,
                                      uint8_t* qhi) {
    if (n < 1 || n > 4 || !lo || !hi || !qlo || !qhi) return -1;
    if (!std::isfinite(p) || !std::isfinite(gap) || gap < 0.0f) return -1;
    double ext = 0.0;
    for (int c = 0; c < n; ++c) {
        if (!std::isfinite(lo[c]) || !std::isfinite(hi[c])) return -1;
        ext = std::max(ext, (double)hi[c] + gap - (double)p);
    }
    int e = ext > 0.0 ? (int)std::ceil(std::log2(ext / 255.0)) : -100;
    e = std::min(std::max(e, -100), 100);
    // a bound with q > 0 lies at least `gap` outside its child's exact bound, in exact arithmetic (the
    // kernels' origin-folded form fma(q, s, p - o) is then conservative, rt_device.h wide_node); q = 0
    // is the corner p itself, which both forms dequantise exactly
    auto lo_ok = [&](uint32_t q, float sc, float l) {
        return deq(p, q, sc) <= l && (q == 0 || (double)p + (double)q * sc <= (double)l - gap);
    };
    auto hi_ok = [&](uint32_t q, float sc, float h) {
        return deq(p, q, sc) >= h && (q == 0 ? (double)p >= h : (double)p + (double)q * sc >= (double)h + gap);
    };
    for (;; ++e) {
        const float sc = std::ldexp(1.0f, e);
        bool ok = true;
        for (int c = 0; c < n && ok; ++c) {
            double fl = std::floor(((double)lo[c] - gap - p) / sc), fh = std::ceil(((double)hi[c] + gap - p) / sc);
            uint32_t a = (uint32_t)std::min(255.0, std::max(0.0, fl));
            uint32_t b = (uint32_t)std::min(255.0, std::max(0.0, fh));
            while (a > 0 && !lo_ok(a, sc, lo[c])) --a;
            while (b < 255 && !hi_ok(b, sc, hi[c])) ++b;
            ok = lo_ok(a, sc, lo[c]) && hi_ok(b, sc, hi[c]);
            qlo[c] = (uint8_t)a;
            qhi[c] = (uint8_t)b;
        }
        if (ok) return e + 127;
        if (e >= 100) return -1;
    }
}

namespace {

// Wide layout of the FAST tree (DevScene::wnodes / wleaves, option "bvh_width" 4): the binary tree
// collapsed to nodes of up to 4 children (the internal child with the largest surface area is
// replaced by its two children while fewer than 4), BFS order, 64 bytes per node:
//   float4 (p.x, p.y, p.z, exponent bytes ex | ey << 8 | ez << 16)    p = the children's lower corner
//   int4   child refs: >= 0 wide node, < 0 leaf ~(64 * rank), INT_MIN = empty slot
//   uint4  (lo.x, lo.y, lo.z, hi.x), uint4 (hi.y, hi.z, 0, 0): one byte per child per word
// A child box dequantises per axis as p + q * 2^(e-127), a superset of the child's exact box, so an
// internal child is never rejected where its leaves would pass.  Leaves, one triangle each, are
// 64-byte records in the reference's DFS rank order (rank = record index, the tie break):
// exact leaf box lo.xyz hi.x | hi.yz a.xy | a.z e1.xyz | e2.xyz triangle index.  The leaf step
// tests the exact box again, so the accepted triangles are those of the binary walk.
void emit_wide(HostScene& hs, const int32_t* L, const int32_t* R, const int32_t* T, const float* box, int64_t nn) {
    hs.wnodes.clear();
    hs.wleaves.clear();
    hs.nwnodes = 0;
    hs.wroot_ref = 0;
    hs.wdepth = 1;
    hs.wdq_omax = 0.0f;
    if (hs.ntri > (1 << 25)) return;   // leaf refs ~(64 * rank) must fit 31 bits: no wide layout
    auto is_inner = [&](int64_t i) { return L[i] >= 0; };
    auto area = [&](int64_t i) {
        const float* b = box + 6 * i;
        const double x = (double)b[3] - b[0], y = (double)b[4] - b[1], z = (double)b[5] - b[2];
        return x * y + y * z + z * x;
    };
    auto kids = [&](int32_t n) {
        std::vector<int32_t> k{L[n], R[n]};
        while (k.size() < 4) {
            int best = -1;
            for (int i = 0; i < (int)k.size(); ++i)
                if (is_inner(k[i]) && (best < 0 || area(k[i]) > area(k[best]))) best = i;
            if (best < 0) break;
            const int32_t c = k[best];
            k[best] = L[c];
            k.insert(k.begin() + best + 1, R[c]);
        }
        return k;
    };
    auto rank_of = [&](int32_t leaf) { return as_i32(hs.tri_geo[12 * (size_t)T[leaf] + 3]); };
    std::vector<int32_t> wide_of(nn, -1), bfs;
    std::vector<std::vector<int32_t>> children;
    if (is_inner(0)) {
        bfs.push_back(0);
        wide_of[0] = 0;
    }
    for (size_t h = 0; h < bfs.size(); ++h) {
        children.push_back(kids(bfs[h]));
        for (int32_t ch : children.back()) {
            if (!is_inner(ch)) continue;
            wide_of[ch] = (int32_t)bfs.size();
            bfs.push_back(ch);
        }
    }
    std::vector<int32_t> need(bfs.size(), 0);
    for (size_t w = bfs.size(); w-- > 0;) {
        int32_t sub = 0;
        for (int32_t ch : children[w])
            if (is_inner(ch)) sub = std::max(sub, need[wide_of[ch]]);
        need[w] = (int32_t)children[w].size() - 1 + sub;
    }
    hs.nwnodes = (int32_t)bfs.size();
    hs.wnodes.assign((size_t)hs.nwnodes * 16, 0.0f);
    int32_t nleaves = 0;
    for (int64_t i = 0; i < nn; ++i)
        if (!is_inner(i) && T[i] >= 0) nleaves = std::max(nleaves, rank_of((int32_t)i) + 1);
    hs.wleaves.assign((size_t)std::max(nleaves, 1) * 16, 0.0f);
    auto leaf_ref = [&](int32_t c) { return ~(64 * rank_of(c)); };
    // the gap of the origin-folded dequantisation: every child bound with q > 0 is
    // quantised at least gap = 2^-17 P outside the exact bound, P = the largest coordinate magnitude of
    // the leaf boxes; that covers the rounding of fma(q, s, p - o) for ray origins up to ~20 P (hit
    // points, and cameras up to DevScene::wdq_omax, checked per frame).  If a node cannot take the gap
    // (no exponent up to 2^100), the whole layout is quantised without it and the exact form runs.
    double pmax = 0.0, bmax = 0.0;   // bmax: the largest |p + q s| the layout holds
    for (int64_t i = 0; i < nn; ++i)
        for (int k = 0; k < 6; ++k) pmax = std::max(pmax, (double)std::fabs(box[6 * i + k]));
    float gap = (std::isfinite(pmax) && pmax > 0x1p-100) ? (float)std::ldexp(pmax, -17) : 0.0f;
    // every node quantises independently: in parallel, with a per-chunk reduction of bmax and of the
    // failure kinds (a node with no room for the gap restarts the whole layout without it)
    auto quantise_all = [&](float g, double* bmax_out) -> int {   // 0 ok, 1 gap failed, 2 no quantisation
        std::atomic<int> fail{0};
        std::mutex mu;
        double bm = 0.0;
        parallel_for((int64_t)bfs.size(), 4096, [&](int64_t w0, int64_t w1) {
            double lbm = 0.0;
            for (int64_t w = w0; w < w1 && fail.load(std::memory_order_relaxed) == 0; ++w) {
                float* o = hs.wnodes.data() + 16 * w;
                const auto& ch = children[w];
                const int n = (int)ch.size();
                float lo[3][4], hi[3][4];
                float p[3];
                for (int a = 0; a < 3; ++a) {
                    p[a] = INFINITY;
                    for (int c = 0; c < n; ++c) {
                        lo[a][c] = box[6 * (int64_t)ch[c] + a];
                        hi[a][c] = box[6 * (int64_t)ch[c] + 3 + a];
                        p[a] = std::min(p[a], lo[a][c]);
                    }
                }
                uint8_t ql[3][4] = {}, qh[3][4] = {};
                uint32_t meta = 0;
                for (int a = 0; a < 3; ++a) {
                    const int ex = rt_debug_quantise_axis(p[a], lo[a], hi[a], n, g, ql[a], qh[a]);
                    if (ex < 0) {
                        fail.store(g > 0.0f ? 1 : 2);
                        return;
                    }
                    meta |= (uint32_t)ex << (8 * a);
                    const double sc = std::ldexp(1.0, ex - 127);
                    for (int c = 0; c < n; ++c)
                        lbm = std::max(lbm, std::max(std::fabs(p[a] + ql[a][c] * sc), std::fabs(p[a] + qh[a][c] * sc)));
                }
                o[0] = p[0]; o[1] = p[1]; o[2] = p[2]; o[3] = as_f32((int32_t)meta);
                for (int c = 0; c < 4; ++c)
                    o[4 + c] = as_f32(c < n ? (is_inner(ch[c]) ? wide_of[ch[c]] : leaf_ref(ch[c])) : INT32_MIN);
                auto pack = [&](const uint8_t* q) {
                    uint32_t v = 0;
                    for (int c = 0; c < 4; ++c) v |= (uint32_t)q[c] << (8 * c);
                    return as_f32((int32_t)v);
                };
                o[8] = pack(ql[0]); o[9] = pack(ql[1]); o[10] = pack(ql[2]); o[11] = pack(qh[0]);
                o[12] = pack(qh[1]); o[13] = pack(qh[2]); o[14] = 0.0f; o[15] = 0.0f;
            }
            std::lock_guard<std::mutex> lk(mu);
            bm = std::max(bm, lbm);
        });
        *bmax_out = bm;
        return fail.load();
    };
    int qf = quantise_all(gap, &bmax);
    if (qf == 1) {   // no room for the gap: quantise without it, exact form only
        gap = 0.0f;
        qf = quantise_all(gap, &bmax);
    }
    if (qf != 0) {   // no containing quantisation: no wide layout (use_wide() keeps the BVH2 walk)
        hs.wnodes.clear();
        hs.wleaves.clear();
        hs.nwnodes = 0;
        hs.wroot_ref = 0;
        hs.wdepth = 1;
        return;
    }
    // origins the gap covers: gap >= u (1 + u) (|p - o| + |p + q s - o| + |b - o|) for every bound, u = 2^-24,
    // with |p|, |b| <= pmax and |p + q s| <= bmax holds for |o| <= (gap / (u (1 + u)) - 2 pmax - bmax) / 3
    // (about 40 pmax); kept 1/2 below that
    {
        const double u = 0x1p-24;
        const double om = gap > 0.0f ? ((double)gap / (u * (1.0 + u)) - 2.0 * pmax - bmax) / 3.0 : 0.0;
        hs.wdq_omax = om > 0.0 ? (float)(0.5 * om) : 0.0f;
    }
    for (int64_t i = 0; i < nn; ++i) {
        if (is_inner(i) || T[i] < 0) continue;
        const int32_t r = rank_of((int32_t)i);
        float* q = hs.wleaves.data() + 16 * (size_t)r;
        const float* b = box + 6 * i;
        const float* g = hs.tri_geo.data() + 12 * (size_t)T[i];
        q[0] = b[0]; q[1] = b[1]; q[2] = b[2]; q[3] = b[3];
        q[4] = b[4]; q[5] = b[5]; q[6] = g[0]; q[7] = g[1];
        q[8] = g[2]; q[9] = g[4]; q[10] = g[5]; q[11] = g[6];
        q[12] = g[8]; q[13] = g[9]; q[14] = g[10]; q[15] = as_f32(T[i]);
    }
    hs.wroot_ref = is_inner(0) ? 0 : leaf_ref(0);
    hs.wdepth = bfs.empty() ? 1 : std::max(1, need[0]);
}

// Emit the FAST node array from a binary tree with one triangle per leaf: internal nodes in BFS
// order, each holding its two children's boxes and refs (rt_internal.h DevScene::nodes).
// box: 6 floats per tree node (lo.xyz, hi.xyz).
void emit_bvh(HostScene& hs, const int32_t* L, const int32_t* R, const int32_t* T, const float* box, int64_t nn) {
    (void)nn;
    auto is_inner = [&](int64_t i) { return L[i] >= 0; };
    std::vector<int32_t> wide_of(nn, -1), bfs;
    if (is_inner(0)) {
        bfs.push_back(0);
        wide_of[0] = 0;
    }
    for (size_t h = 0; h < bfs.size(); ++h) {
        for (int32_t ch : {L[bfs[h]], R[bfs[h]]}) {
            if (!is_inner(ch)) continue;
            wide_of[ch] = (int32_t)bfs.size();
            bfs.push_back(ch);
        }
    }
    // stack bound: a node pushes one entry at most; need = max over root-to-leaf paths of the sum
    // (children are after their parents in BFS order: sweep backwards)
    std::vector<int32_t> need(bfs.size(), 0);
    for (size_t w = bfs.size(); w-- > 0;) {
        int32_t sub = 0;
        for (int32_t ch : {L[bfs[w]], R[bfs[w]]})
            if (is_inner(ch)) sub = std::max(sub, need[wide_of[ch]]);
        need[w] = 1 + sub;
    }
    constexpr int F = 4 * rt::kNodeF4;   // floats per node
    // the FAST traversal's triangle records (DevScene::tri_fast), in the order a depth-first walk of
    // this tree meets its leaves: pos[t] = record of t
    std::vector<int32_t> pos((size_t)hs.ntri, -1);
    {
        int32_t next = 0;
        auto place = [&](int32_t c) {
            if (!is_inner(c) && T[c] >= 0 && pos[T[c]] < 0) pos[T[c]] = next++;
        };
        if (is_inner(0)) {
            std::vector<int32_t> st{0};
            while (!st.empty()) {
                const int32_t n = st.back();
                st.pop_back();
                place(L[n]);
                place(R[n]);
                if (is_inner(R[n])) st.push_back(R[n]);
                if (is_inner(L[n])) st.push_back(L[n]);
            }
        }
        if (!is_inner(0)) place(0);
        for (int32_t t = 0; t < hs.ntri; ++t)
            if (pos[t] < 0) pos[t] = next++;   // unreachable triangles keep their order
        hs.tri_fast.assign(hs.tri_geo.size(), 0.0f);
        for (int32_t t = 0; t < hs.ntri; ++t)
            for (int k = 0; k < 12; ++k) hs.tri_fast[12 * (size_t)pos[t] + k] = hs.tri_geo[12 * (size_t)t + k];
    }
    hs.nnodes = (int32_t)bfs.size();
    hs.nodes.assign((size_t)hs.nnodes * F, 0.0f);
    for (size_t w = 0; w < bfs.size(); ++w) {
        float* o = hs.nodes.data() + (size_t)F * w;
        const int32_t n = bfs[w];
        auto ref = [&](int32_t c) { return is_inner(c) ? wide_of[c] : ~(48 * pos[T[c]]); };
        const float* c0 = box + 6 * (int64_t)L[n];
        const float* c1 = box + 6 * (int64_t)R[n];
        o[0] = c0[0]; o[1] = c0[3]; o[2] = c0[1]; o[3] = c0[4];
        o[4] = c1[0]; o[5] = c1[3]; o[6] = c1[1]; o[7] = c1[4];
        o[8] = c0[2]; o[9] = c0[5]; o[10] = c1[2]; o[11] = c1[5];
        o[12] = as_f32(ref(L[n])); o[13] = as_f32(ref(R[n])); o[14] = 0.0f; o[15] = 0.0f;
    }
    hs.root_ref = is_inner(0) ? 0 : ~(48 * pos[T[0]]);
    for (int k = 0; k < 6; ++k) hs.root_box[k] = box[k];
    hs.depth = bfs.empty() ? 1 : std::max(1, need[0]);
    emit_wide(hs, L, R, T, box, nn);
}

// The clustered form of the brute-force boxes (HostScene::brute_cbox / brute_crow; option "brute_cluster",
// mode 0 off, < 0 auto, > 0 force): the SAH regrouping of the distinct leaf boxes is cut, top-down, into
// subtrees of 2..kClusterSlots boxes that become clusters -- mode auto: where the estimated cost of one
// union test plus the passing rays' compacted items is clearly below the subtree's lock-step tests
// (rt_layout.h kClusterKappa, kClusterGain; p = the union's surface area over the root's, the chance that
// a ray through the scene crosses it); mode force: every such subtree -- and single slots.
// brute_cbox: the single slots in brute_box order, padded with pad_box() to whole groups of kBoxGroup, then
// kClusterSlots slots per cluster (its boxes in brute_box order, padded likewise).  A cluster's row holds the
// componentwise minimum / maximum of its members' bounds (one ulp further out where a flat member lies on
// it, below): slab() is monotone in the bounds, so a ray that passes a member passes the union.  Clusters
// hold finite boxes only.  brute_box itself is untouched.
void build_clusters(HostScene& hs, int mode) {
    hs.brute_cbox.clear();
    hs.brute_crow.clear();
    hs.ncluster = 0;
    hs.nsingle = 0;
    const int32_t n = hs.nbox;
    if (mode == 0 || n < 2) return;
    std::vector<float> lb(6 * (size_t)n);
    std::vector<int32_t> ids((size_t)n);
    for (int32_t g = 0; g < n; ++g) {
        const float* b = hs.brute_box.data() + 8 * (size_t)g;
        float* o = lb.data() + 6 * (size_t)g;
        o[0] = b[0]; o[1] = b[2]; o[2] = b[4]; o[3] = b[1]; o[4] = b[3]; o[5] = b[5];
        ids[g] = g;
    }
    rt::SahTree st;
    rt::sah_build(lb.data(), ids.data(), n, st);
    std::vector<int32_t> cnt(st.L.size(), 0);
    std::function<int32_t(int32_t)> count = [&](int32_t i) {
        return cnt[i] = st.L[i] < 0 ? 1 : count(st.L[i]) + count(st.R[i]);
    };
    count(0);
    auto area = [&](int32_t i) {
        const float* b = st.box.data() + 6 * (size_t)i;
        const double x = (double)b[3] - b[0], y = (double)b[4] - b[1], z = (double)b[5] - b[2];
        return x * y + y * z + z * x;
    };
    std::function<void(int32_t, std::vector<int32_t>&)> collect = [&](int32_t i, std::vector<int32_t>& out) {
        if (st.L[i] < 0) {
            out.push_back(st.leaf[i]);
            return;
        }
        collect(st.L[i], out);
        collect(st.R[i], out);
    };
    const double root = area(0);
    std::vector<int32_t> singles;
    std::vector<std::vector<int32_t>> clusters;
    std::function<void(int32_t)> cut = [&](int32_t i) {
        if (st.L[i] < 0) {
            singles.push_back(st.leaf[i]);
            return;
        }
        const int32_t m = cnt[i];
        if (m <= rt::kClusterSlots) {
            std::vector<int32_t> mem;
            collect(i, mem);
            bool take = true;
            for (int32_t g : mem)
                for (int k = 0; k < 6; ++k) take = take && std::isfinite(hs.brute_box[8 * (size_t)g + k]);
            if (take && mode < 0) {
                const double p = root > 0.0 && std::isfinite(root) ? std::min(1.0, area(i) / root) : 1.0;
                take = 1.0 + rt::kClusterKappa * p * rt::kClusterSlots < rt::kClusterGain * m;
            }
            if (take) {
                std::sort(mem.begin(), mem.end());
                clusters.push_back(mem);
                return;
            }
        }
        cut(st.L[i]);
        cut(st.R[i]);
    };
    cut(0);
    if (clusters.empty()) return;
    std::sort(singles.begin(), singles.end());
    std::sort(clusters.begin(), clusters.end());
    const size_t ns4 = (singles.size() + rt::kBoxGroup - 1) / rt::kBoxGroup * rt::kBoxGroup;
    const size_t nslot = ns4 + clusters.size() * rt::kClusterSlots;
    hs.brute_cbox.assign(8 * nslot, 0.0f);
    for (size_t s = 0; s < nslot; ++s) pad_box(hs.brute_cbox.data() + 8 * s);
    auto put = [&](size_t s, int32_t g) {
        std::memcpy(hs.brute_cbox.data() + 8 * s, hs.brute_box.data() + 8 * (size_t)g, 8 * sizeof(float));
    };
    for (size_t s = 0; s < singles.size(); ++s) put(s, singles[s]);
    hs.brute_crow.assign(8 * clusters.size(), 0.0f);
    for (size_t c = 0; c < clusters.size(); ++c) {
        const size_t first = ns4 + c * rt::kClusterSlots;
        float* r = hs.brute_crow.data() + 8 * c;
        for (size_t j = 0; j < clusters[c].size(); ++j) {
            put(first + j, clusters[c][j]);
            const float* b = hs.brute_box.data() + 8 * (size_t)clusters[c][j];
            for (int k = 0; k < 6; ++k)
                r[k] = j == 0 ? b[k] : (k & 1) ? std::max(r[k], b[k]) : std::min(r[k], b[k]);
        }
        // a member that is flat on an axis (lo = hi = v: an axis-aligned face) passes a ray that lies in its
        // plane with a zero direction component there: both its slab distances are 0 * inf = NaN and the axis
        // drops out.  A union bound equal to v would give that ray one NaN and one infinite distance, and
        // reject it; one ulp further out both distances are infinite, of opposite signs, and the axis drops
        // out of the union test as well
        for (int32_t g : clusters[c]) {
            const float* b = hs.brute_box.data() + 8 * (size_t)g;
            for (int a = 0; a < 3; ++a) {
                if (b[2 * a] != b[2 * a + 1]) continue;
                if (r[2 * a] == b[2 * a]) r[2 * a] = std::nextafterf(r[2 * a], -INFINITY);
                if (r[2 * a + 1] == b[2 * a]) r[2 * a + 1] = std::nextafterf(r[2 * a + 1], INFINITY);
            }
        }
        r[6] = as_f32((int32_t)first);
        r[7] = as_f32((int32_t)clusters[c].size());
    }
    hs.ncluster = (int32_t)clusters.size();
    hs.nsingle = (int32_t)singles.size();
}

// Near-safe boxes (option "brute_near", HostScene::brute_near; the proof is DESIGN.md 4.2): slot b (8 floats of
// brute_box's form) is flat on exactly one axis a at a finite h, a proper finite range on the other two, and each
// of its one or two records, as the kernel reads it from hs.brute, lies in that plane -- p0[a] == h, e1[a] and
// e2[a] zero -- with an in-plane cross product N = e1[b] e2[c] - e1[c] e2[b] that is not zero and cancels by at
// most kNearKappa, every non-zero component and bound within 2^+-kNearExp.  Then Moller-Trumbore's k on such a
// record is the box's own plane distance to a relative 2^-13.9, whatever the ray: a pass closer than kNearFloor is
// no hit.  Evaluated in double, in which the products of two floats and the comparisons below are exact.
bool near_safe(const HostScene& hs, const float* b) {
    int nf = 0, ax = -1;
    const double lim_lo = std::ldexp(1.0, -rt::kNearExp), lim_hi = std::ldexp(1.0, rt::kNearExp);
    auto in_range = [&](double v) { return v == 0.0 || (std::fabs(v) >= lim_lo && std::fabs(v) <= lim_hi); };
    for (int a = 0; a < 3; ++a) {
        if (!std::isfinite(b[2 * a]) || !std::isfinite(b[2 * a + 1])) return false;
        if (!in_range(b[2 * a]) || !in_range(b[2 * a + 1])) return false;
        if (b[2 * a] == b[2 * a + 1]) { ++nf; ax = a; }
        else if (!(b[2 * a] < b[2 * a + 1])) return false;
    }
    if (nf != 1) return false;
    const double h = b[2 * ax];
    const int u = (ax + 1) % 3, v = (ax + 2) % 3;
    int32_t q[2];
    std::memcpy(q, b + 6, 8);
    for (int j = 0; j < 2; ++j) {
        if (j == 1 && q[1] < 0) break;
        if (q[j] < 0 || q[j] >= hs.nbrute) return false;
        const float* r = hs.brute.data() + 16 * (size_t)q[j];
        const float *p0 = r + 6, *e1 = r + 9, *e2 = r + 12;
        for (int k = 0; k < 3; ++k)
            if (!std::isfinite(p0[k]) || !std::isfinite(e1[k]) || !std::isfinite(e2[k]) || !in_range(p0[k]) ||
                !in_range(e1[k]) || !in_range(e2[k]))
                return false;
        if ((double)p0[ax] != h || e1[ax] != 0.0f || e2[ax] != 0.0f) return false;
        const double t1 = (double)e1[u] * e2[v], t2 = (double)e1[v] * e2[u], N = t1 - t2;
        if (N == 0.0 || !((std::fabs(t1) + std::fabs(t2)) <= rt::kNearKappa * std::fabs(N))) return false;
    }
    return true;
}

// A split wall (option "brute_quad"; rule, bound and proof: DESIGN.md 4.2).  Face slot b of shell box S (6 bounds)
// is split when it is near-safe, lists two records whose vertices p0, p0 + e1, p0 + e2 are exact in double, every
// component within 2^+-kQuadExp, cancellation at most kQuadKappa, and there is an edge coordinate l1 (u, v or
// 1 - u - v) of the first record and one l2 of the second with l1 = s sigma / r1 and l2 = -s sigma / r2 to within
// kQuadSlack at the four corners of the face -- so over all of it, the functions being affine -- where sigma(P) =
// A . P + gamma is the line with float coefficients the kernel evaluates, s = +-1, and r1, r2 in [1, kQuadRatio]
// are the triangles' heights over the line in units of the smaller one.  The first non-zero component of A is
// positive; side = the first record lies on sigma >= 0.  Last, kQuadBand must be kQuadSafety times the wall's error
// bound (quad_bound below, restated in tests/test_brute_quad.py).  Every doubt: not split.
struct QuadLine { float A[3] = {0, 0, 0}; float gamma = 0; int side = 0; };
bool quad_split(const HostScene& hs, const float* b, const float* S, QuadLine& out) {
    if (!near_safe(hs, b)) return false;
    int32_t q[2];
    std::memcpy(q, b + 6, 8);
    if (q[1] < 0) return false;
    int a = 0;
    for (int k = 0; k < 3; ++k) if (b[2 * k] == b[2 * k + 1]) a = k;
    const int ax[2] = {(a + 1) % 3, (a + 2) % 3};
    const double lo = std::ldexp(1.0, -rt::kQuadExp), hi = std::ldexp(1.0, rt::kQuadExp);
    auto in_range = [&](double v) { return v == 0.0 || (std::fabs(v) >= lo && std::fabs(v) <= hi); };
    for (int k = 0; k < 6; ++k) if (!in_range(S[k])) return false;
    const double eps = std::ldexp(1.0, -24) * (1.0 + std::ldexp(1.0, -10));
    double W[2], Cm[2], corner[4][2];
    for (int j = 0; j < 2; ++j) {
        W[j] = (double)S[2 * ax[j] + 1] - (double)S[2 * ax[j]];
        Cm[j] = std::max(std::fabs((double)S[2 * ax[j]]), std::fabs((double)S[2 * ax[j] + 1]));
    }
    for (int c = 0; c < 4; ++c) {
        corner[c][0] = S[2 * ax[0] + (c & 1)];
        corner[c][1] = S[2 * ax[1] + (c >> 1)];
    }
    // the two triangles' edge coordinates as affine functions g0 P[0] + g1 P[1] + c of the in-plane point, their
    // bounds over the face and Moller-Trumbore's error on each (quad_bound)
    struct Coord { double g[2], c, err; };
    Coord L[2][3];
    double V[2][3][2];
    for (int t = 0; t < 2; ++t) {
        const float* r = hs.brute.data() + 16 * (size_t)q[t];
        double p0[2], e1[2], e2[2];
        for (int j = 0; j < 2; ++j) {
            p0[j] = r[6 + ax[j]]; e1[j] = r[9 + ax[j]]; e2[j] = r[12 + ax[j]];
            if (!in_range(p0[j]) || !in_range(e1[j]) || !in_range(e2[j])) return false;
            const double s1 = p0[j] + e1[j], s2 = p0[j] + e2[j];
            if (s1 - p0[j] != e1[j] || s1 - e1[j] != p0[j] || s2 - p0[j] != e2[j] || s2 - e2[j] != p0[j]) return false;
            V[t][0][j] = p0[j]; V[t][1][j] = s1; V[t][2][j] = s2;
        }
        const double t1 = e1[0] * e2[1], t2 = e1[1] * e2[0], N = t1 - t2;
        if (N == 0.0 || !((std::fabs(t1) + std::fabs(t2)) <= rt::kQuadKappa * std::fabs(N))) return false;
        // u = ((P - p0) x e2) / N, v = (e1 x (P - p0)) / N in the plane
        Coord& u = L[t][0]; Coord& v = L[t][1]; Coord& w = L[t][2];
        u.g[0] = e2[1] / N; u.g[1] = -e2[0] / N; u.c = -(p0[0] * e2[1] - p0[1] * e2[0]) / N;
        v.g[0] = -e1[1] / N; v.g[1] = e1[0] / N; v.c = -(e1[0] * p0[1] - e1[1] * p0[0]) / N;
        w.g[0] = -u.g[0] - v.g[0]; w.g[1] = -u.g[1] - v.g[1]; w.c = 1.0 - u.c - v.c;
        double mx[2] = {0.0, 0.0};
        for (int k = 0; k < 2; ++k)
            for (int c = 0; c < 4; ++c)
                mx[k] = std::max(mx[k], std::fabs(L[t][k].g[0] * corner[c][0] + L[t][k].g[1] * corner[c][1] + L[t][k].c));
        const double Qu = (W[0] * std::fabs(e2[1]) + W[1] * std::fabs(e2[0])) / std::fabs(N);
        const double Qv = (W[0] * std::fabs(e1[1]) + W[1] * std::fabs(e1[0])) / std::fabs(N);
        u.err = eps * (24.0 * mx[0] + 16.0 * Qu);
        v.err = eps * (24.0 * mx[1] + 16.0 * Qv);
        w.err = u.err + v.err + eps * (mx[0] + mx[1]);
    }
    auto at = [](const Coord& l, const double* P) { return l.g[0] * P[0] + l.g[1] * P[1] + l.c; };
    for (int k1 = 0; k1 < 3; ++k1) {
        const Coord& l1 = L[0][k1];
        double mu = 0.0;
        bool ok = true;
        for (int j = 0; j < 3; ++j) {
            const double x = at(l1, V[1][j]);
            ok = ok && x <= rt::kQuadSlack;
            mu = std::max(mu, -x);
        }
        if (!ok || !(mu > 0.0)) continue;
        const double r1 = std::max(1.0, 1.0 / mu), r2 = std::max(1.0, mu);
        if (!(r1 <= rt::kQuadRatio && r2 <= rt::kQuadRatio)) continue;
        QuadLine ln;
        ln.A[ax[0]] = (float)(r1 * l1.g[0]);
        ln.A[ax[1]] = (float)(r1 * l1.g[1]);
        ln.gamma = (float)(r1 * l1.c);
        ln.side = 1;
        for (int k = 0; k < 3; ++k) {
            if (ln.A[k] == 0.0f) continue;
            if (ln.A[k] < 0.0f) {
                for (int m = 0; m < 3; ++m) ln.A[m] = -ln.A[m];
                ln.gamma = -ln.gamma;
                ln.side = 0;
            }
            break;
        }
        const double s = ln.side ? 1.0 : -1.0, A0 = ln.A[ax[0]], A1 = ln.A[ax[1]], G = ln.gamma;
        auto sigma = [&](const double* P) { return A0 * P[0] + A1 * P[1] + G; };
        for (int c = 0; c < 4; ++c) ok = ok && std::fabs(at(l1, corner[c]) - s * sigma(corner[c]) / r1) <= rt::kQuadSlack;
        if (!ok) continue;
        for (int k2 = 0; k2 < 3; ++k2) {
            const Coord& l2 = L[1][k2];
            bool ok2 = true;
            for (int c = 0; c < 4; ++c) ok2 = ok2 && std::fabs(at(l2, corner[c]) + s * sigma(corner[c]) / r2) <= rt::kQuadSlack;
            if (!ok2) continue;
            // quad_bound: the classifier's error on sigma~, then each dropped record's
            const double Ms = std::fabs(A0) * Cm[0] + std::fabs(A1) * Cm[1] + std::fabs(G);
            const double Ecls = eps * (std::fabs(A0) * (4.0 * W[0] + Cm[0]) + std::fabs(A1) * (4.0 * W[1] + Cm[1]) + 3.0 * Ms);
            const double E = std::max(Ecls + r1 * (rt::kQuadSlack + l1.err), Ecls + r2 * (rt::kQuadSlack + l2.err));
            if (!((double)rt::kQuadBand >= rt::kQuadSafety * E)) return false;
            out = ln;
            return true;
        }
    }
    return false;
}

// The shell of a clustered scene (HostScene::brute_shell; option "brute_shell", mode 0 off, < 0 auto, > 0 force):
// a box S with lo < hi, finite, on every axis, and the single slots that are faces of it -- a slot is a face when
// its box is flat on one axis at S's lower or upper bound there and equals S's range on the other two, every
// equality bitwise (-0 is not +0).  The walls of an axis-aligned room are such slots: their 6 bounds each are
// drawn from S's 6, so the kernel computes S's six plane distances once per ray and tests each face from them
// (rt_device.h trace_brute_compact).  Two faces fix S, so every shell of two or more faces is the S of some pair
// of flat singles: perpendicular ones (each lies on an end of the other's range along its flat axis, and their
// ranges on the third axis agree) or parallel ones (the same ranges on the other two axes).  The S with the most
// faces is taken; among equals the one whose faces' slots, in ascending order, compare lowest, then the lowest
// bounds' bits.  A face position holds the first slot that fits (bit-identical boxes share a slot, so a second
// one is a third coplanar record: it stays a single).  auto: only from kShellMinFaces faces; force: from the two
// that define a shell.  brute_cbox, brute_crow and nsingle are untouched; the singles that are no face are copied
// behind the record in their order.
void build_shell(HostScene& hs, int mode, int quad) {
    hs.brute_shell.clear();
    hs.nshell = 0;
    hs.nrest = 0;
    hs.shell_floor = 0.0f;
    hs.shell_mask = 0;
    hs.nquad = 0;
    if (mode == 0 || hs.ncluster == 0) return;
    const int32_t n = hs.nsingle;
    auto bits = [](float f) {
        uint32_t u;
        std::memcpy(&u, &f, 4);
        return u;
    };
    auto same = [&](float a, float b) { return bits(a) == bits(b); };
    auto box = [&](int32_t s) { return hs.brute_cbox.data() + 8 * (size_t)s; };
    // the axis a slot is flat on, when it is flat on one axis alone and a proper finite range on the others
    std::vector<int> flat((size_t)n, -1);
    for (int32_t s = 0; s < n; ++s) {
        const float* b = box(s);
        int nf = 0, ax = -1;
        bool ok = true;
        for (int a = 0; a < 3; ++a) {
            ok = ok && std::isfinite(b[2 * a]) && std::isfinite(b[2 * a + 1]);
            if (same(b[2 * a], b[2 * a + 1])) { ++nf; ax = a; }
            else ok = ok && b[2 * a] < b[2 * a + 1];
        }
        if (ok && nf == 1) flat[s] = ax;
    }
    typedef std::array<uint32_t, 6> Key;          // S's bounds' bits, lo.x hi.x lo.y hi.y lo.z hi.z
    std::map<Key, std::array<int32_t, 6>> shells;   // -> the slot at each face position -x +x -y +y -z +z, or -1
    auto add_face = [&](std::array<int32_t, 6>& f, const float* S, int32_t s) {
        const int a = flat[s];
        const int pos = 2 * a + (same(box(s)[2 * a], S[2 * a]) ? 0 : 1);
        if (f[pos] < 0 || s < f[pos]) f[pos] = s;
    };
    for (int32_t s = 0; s < n; ++s) {
        if (flat[s] < 0) continue;
        for (int32_t t = s + 1; t < n; ++t) {
            if (flat[t] < 0) continue;
            const float *p = box(s), *q = box(t);
            const int a = flat[s], b = flat[t];
            float S[6];
            if (a == b) {
                bool ok = !same(p[2 * a], q[2 * a]);
                for (int k = 0; k < 3; ++k)
                    if (k != a) ok = ok && same(p[2 * k], q[2 * k]) && same(p[2 * k + 1], q[2 * k + 1]);
                if (!ok) continue;
                for (int k = 0; k < 6; ++k) S[k] = p[k];
                S[2 * a] = std::min(p[2 * a], q[2 * a]);
                S[2 * a + 1] = std::max(p[2 * a], q[2 * a]);
                if (!(S[2 * a] < S[2 * a + 1])) continue;   // -0 and +0: no range
            } else {
                const int c = 3 - a - b;
                if (!(same(p[2 * a], q[2 * a]) || same(p[2 * a], q[2 * a + 1]))) continue;
                if (!(same(q[2 * b], p[2 * b]) || same(q[2 * b], p[2 * b + 1]))) continue;
                if (!(same(p[2 * c], q[2 * c]) && same(p[2 * c + 1], q[2 * c + 1]))) continue;
                S[2 * a] = q[2 * a]; S[2 * a + 1] = q[2 * a + 1];
                S[2 * b] = p[2 * b]; S[2 * b + 1] = p[2 * b + 1];
                S[2 * c] = p[2 * c]; S[2 * c + 1] = p[2 * c + 1];
            }
            Key key;
            for (int k = 0; k < 6; ++k) key[k] = bits(S[k]);
            auto it = shells.find(key);
            if (it == shells.end()) it = shells.emplace(key, std::array<int32_t, 6>{-1, -1, -1, -1, -1, -1}).first;
            add_face(it->second, S, s);
            add_face(it->second, S, t);
        }
    }
    const Key* best = nullptr;
    std::vector<int32_t> best_slots;
    for (const auto& kv : shells) {
        std::vector<int32_t> slots;
        for (int32_t s : kv.second)
            if (s >= 0) slots.push_back(s);
        std::sort(slots.begin(), slots.end());
        if (!best || slots.size() > best_slots.size() || (slots.size() == best_slots.size() && slots < best_slots)) {
            best = &kv.first;
            best_slots = slots;
        }
    }
    const int need = mode < 0 ? rt::kShellMinFaces : 2;
    if (!best || (int)best_slots.size() < need) return;
    const std::array<int32_t, 6>& face = shells[*best];
    const int32_t nrest = n - (int32_t)best_slots.size();
    const size_t nr4 = ((size_t)nrest + rt::kBoxGroup - 1) / rt::kBoxGroup * rt::kBoxGroup;
    hs.brute_shell.assign(rt::kShellRecF + 8 * nr4, 0.0f);
    float* r = hs.brute_shell.data();
    for (int k = 0; k < 6; ++k) std::memcpy(r + k, &(*best)[k], 4);
    r[6] = as_f32(nrest);
    r[7] = as_f32((int32_t)best_slots.size());
    for (int f = 0; f < 6; ++f) {
        r[8 + 2 * f] = face[f] < 0 ? as_f32(-1) : box(face[f])[6];
        r[9 + 2 * f] = face[f] < 0 ? as_f32(-1) : box(face[f])[7];
    }
    // the rows (rt_layout.h kShellRows): each face's packed records, and its line where it is split
    float S6[6];
    for (int k = 0; k < 6; ++k) std::memcpy(S6 + k, &(*best)[k], 4);
    for (int f = 0; f < rt::kShellRows; ++f) {
        float* row = r + 4 * rt::kShellRowF4 + 8 * f;
        uint32_t both = ~0u, pos = ~0u, neg = ~0u, flags = 0;
        if (f < 6 && face[f] >= 0) {
            const uint32_t q0 = (uint32_t)as_i32(box(face[f])[6]), q1 = (uint32_t)as_i32(box(face[f])[7]);
            // records are queued as 16-bit ranks (the ring's entries): brute_max is far below 0xffff
            both = pos = neg = (q0 & 0xffffu) | (q1 << 16);
            QuadLine ln;
            if (quad != 0 && q1 < 0xffffu && quad_split(hs, box(face[f]), S6, ln)) {
                for (int k = 0; k < 3; ++k) row[k] = ln.A[k];
                row[3] = ln.gamma;
                pos = (ln.side ? q0 : q1) | 0xffff0000u;
                neg = (ln.side ? q1 : q0) | 0xffff0000u;
                flags = 1u | (ln.side ? 2u : 0u);
                ++hs.nquad;
            }
        }
        row[4] = as_f32((int32_t)both); row[5] = as_f32((int32_t)pos);
        row[6] = as_f32((int32_t)neg); row[7] = as_f32((int32_t)flags);
    }
    // the number of split faces above the face count: the kernels read it as the rule's enable
    r[7] = as_f32((int32_t)best_slots.size() | (hs.nquad << 8));
    float* o = r + rt::kShellRecF;
    for (size_t s = 0; s < nr4; ++s) pad_box(o + 8 * s);
    for (int32_t s = 0; s < n; ++s)
        if (!std::binary_search(best_slots.begin(), best_slots.end(), s)) {
            std::memcpy(o, box(s), 8 * sizeof(float));
            o += 8;
        }
    hs.nshell = (int32_t)best_slots.size();
    hs.nrest = nrest;
    // one floor for all the face tests (option "brute_near"): only when every face present is near-safe
    bool near = true;
    for (int32_t s : best_slots) near = near && near_safe(hs, box(s));
    hs.shell_floor = near ? rt::kNearFloor : 0.0f;
    // the faces' boxes in brute_box, by their first record (a record belongs to one box)
    for (int32_t s : best_slots)
        for (int32_t g = 0; g < hs.nbox && g < 64; ++g)
            if (as_i32(hs.brute_box[8 * (size_t)g + 6]) == as_i32(box(s)[6])) hs.shell_mask |= 1ull << g;
}

// Pack the FAST layout from the reference export.  Returns false (with
// reason) if the export is not a proper binary tree with one triangle per
// leaf, in which case only the REF traversal is available.  layout
// RT_BVH_REFERENCE keeps the reference's tree, RT_BVH_SAH regroups its leaf
// boxes (bvh_sah.cpp); both give the same hits.
bool pack_fast(HostScene& hs, const float* bvh9, int64_t nn, int64_t ntri, int layout, int brute_max, int cluster,
               int shell, int quad, std::string& why) {
    if (nn <= 0) {
        why = "empty BVH";
        return false;
    }
    if (ntri > 0x7fffffff / 48) {  // leaf refs are ~(48 * triangle)
        why = "more than 44.7M triangles";
        return false;
    }
    std::vector<int32_t> L(nn), R(nn), T(nn);
    for (int64_t i = 0; i < nn; ++i) {
        if (!fidx(bvh9[9 * i + 0], nn, &L[i]) || !fidx(bvh9[9 * i + 1], nn, &R[i]) ||
            !fidx(bvh9[9 * i + 8], ntri, &T[i])) {
            why = "index out of range";
            return false;
        }
    }
    // Check the tree shape over the reachable nodes.
    std::vector<uint8_t> seen(nn, 0);
    auto is_leaf = [&](int64_t i) { return L[i] == -1 && R[i] == -1 && T[i] >= 0; };
    auto is_inner = [&](int64_t i) { return L[i] >= 0 && R[i] >= 0 && T[i] == -1; };
    if (!is_leaf(0) && !is_inner(0)) {
        why = "root is neither a one-triangle leaf nor a two-child node";
        return false;
    }
    std::vector<int32_t> tri_seen(ntri, 0), leaves;
    std::vector<int32_t> queue{0};
    seen[0] = 1;
    for (size_t h = 0; h < queue.size(); ++h) {
        const int32_t n = queue[h];
        if (is_leaf(n)) {
            if (tri_seen[T[n]]++) {
                why = "triangle in two leaves";
                return false;
            }
            leaves.push_back(n);
            continue;
        }
        if (!is_inner(n)) {
            why = "node with one child, or with both a triangle and children";
            return false;
        }
        for (int32_t ch : {L[n], R[n]}) {
            if (seen[ch]) {
                why = "node reachable twice (not a tree)";
                return false;
            }
            seen[ch] = 1;
            queue.push_back(ch);
        }
    }
    // Rank of each leaf triangle in the reference visiting order: pre-order
    // DFS, right child first (push left then right, MathLib.cl:269-276).
    std::vector<int32_t> rank(ntri, 0x7fffffff);
    {
        std::vector<int32_t> st;
        st.push_back(0);
        int32_t r = 0;
        while (!st.empty()) {
            const int32_t n = st.back();
            st.pop_back();
            if (T[n] >= 0) rank[T[n]] = r++;
            if (L[n] >= 0) st.push_back(L[n]);
            if (R[n] >= 0) st.push_back(R[n]);
        }
    }
    for (int64_t t = 0; t < ntri; ++t) {
        hs.tri_geo[12 * t + 3] = as_f32(rank[t]);
        hs.tri_geo[12 * t + 7] = as_f32((int32_t)t);   // e1.w: the triangle's own index (FAST hit records)
    }
    // small scenes: brute-force records of the reachable triangles in DFS-rank order
    hs.brute.clear();
    hs.brute_box.clear();
    hs.nbrute = 0;
    hs.nbox = 0;
    hs.brute_cbox.clear();
    hs.brute_crow.clear();
    hs.ncluster = 0;
    hs.nsingle = 0;
    hs.brute_shell.clear();
    hs.nshell = 0;
    hs.nrest = 0;
    hs.brute_near.clear();
    hs.shell_floor = 0.0f;
    hs.shell_mask = 0;
    hs.nquad = 0;
    if ((int64_t)leaves.size() <= (int64_t)brute_max) {
        std::vector<int32_t> by_rank(leaves.size());
        for (int32_t n : leaves) by_rank[rank[T[n]]] = n;
        hs.brute.assign(16 * by_rank.size(), 0.0f);
        for (size_t q = 0; q < by_rank.size(); ++q) {
            const float* nd = bvh9 + 9 * (int64_t)by_rank[q];
            const int32_t t = T[by_rank[q]];
            const float* g = hs.tri_geo.data() + 12 * t;
            float* r = hs.brute.data() + 16 * q;
            r[0] = nd[2]; r[1] = nd[3]; r[2] = nd[4]; r[3] = nd[5];      // lo.xyz hi.x
            r[4] = nd[6]; r[5] = nd[7]; r[6] = g[0]; r[7] = g[1];        // hi.yz a.xy
            r[8] = g[2]; r[9] = g[4]; r[10] = g[5]; r[11] = g[6];        // a.z e1.xyz
            r[12] = g[8]; r[13] = g[9]; r[14] = g[10]; r[15] = as_f32(t); // e2.xyz tri
        }
        hs.nbrute = (int32_t)by_rank.size();
        // the distinct leaf boxes, 32 bytes each: records whose leaf boxes are bit-identical (the
        // two triangles of an axis-aligned or vertical quad) share one box test, which passes or
        // fails for both.  Each box lists up to two records (the second -1 when alone); padded with
        // pad_box() to whole groups of rt::kBoxGroup (the lock-step loop loads a group with one
        // scalar wait).
        std::vector<std::array<int32_t, 2>> groups;
        {
            std::map<std::array<uint32_t, 6>, size_t> open;   // box bits -> group with a free slot
            for (size_t q = 0; q < by_rank.size(); ++q) {
                const float* r = hs.brute.data() + 16 * q;
                std::array<uint32_t, 6> key;
                for (int k = 0; k < 6; ++k) std::memcpy(&key[k], r + k, 4);
                auto it = open.find(key);
                if (it != open.end()) {
                    groups[it->second][1] = (int32_t)q;
                    open.erase(it);
                } else {
                    open[key] = groups.size();
                    groups.push_back({(int32_t)q, -1});
                }
            }
        }
        hs.nbox = (int32_t)groups.size();
        const size_t ng = (groups.size() + rt::kBoxGroup - 1) / rt::kBoxGroup * rt::kBoxGroup;
        hs.brute_box.assign(8 * ng, 0.0f);
        for (size_t g = 0; g < ng; ++g) {
            float* b = hs.brute_box.data() + 8 * g;
            if (g < groups.size()) {
                const float* r = hs.brute.data() + 16 * groups[g][0];   // lo.xyz hi.x | hi.yz ...
                b[0] = r[0]; b[1] = r[3];                                // lo.x hi.x
                b[2] = r[1]; b[3] = r[4];                                // lo.y hi.y
                b[4] = r[2]; b[5] = r[5];                                // lo.z hi.z
                b[6] = as_f32(groups[g][0]); b[7] = as_f32(groups[g][1]);
            } else {
                pad_box(b);
            }
        }
        hs.brute_near.assign((size_t)hs.nbox, 0);
        for (int32_t g = 0; g < hs.nbox; ++g) hs.brute_near[g] = near_safe(hs, hs.brute_box.data() + 8 * (size_t)g);
        build_clusters(hs, cluster);
        build_shell(hs, shell, quad);
    }
    if (layout == RT_BVH_SAH && leaves.size() > 1) {
        std::vector<float> lb(6 * leaves.size());
        std::vector<int32_t> ids(leaves.size());
        for (size_t q = 0; q < leaves.size(); ++q) {
            const float* nd = bvh9 + 9 * (int64_t)leaves[q];
            for (int k = 0; k < 6; ++k) lb[6 * q + k] = nd[2 + k];
            ids[q] = T[leaves[q]];
        }
        rt::SahTree st;
        rt::sah_build(lb.data(), ids.data(), (int64_t)leaves.size(), st);
        emit_bvh(hs, st.L.data(), st.R.data(), st.leaf.data(), st.box.data(), (int64_t)st.L.size());
        return true;
    }
    std::vector<float> box(6 * nn);
    for (int64_t i = 0; i < nn; ++i)
        for (int k = 0; k < 6; ++k) box[6 * i + k] = bvh9[9 * i + 2 + k];
    emit_bvh(hs, L.data(), R.data(), T.data(), box.data(), nn);
    return true;
}

}  // namespace

namespace rt {

bool shell_direct(HostScene& hs, int direct) {
    if (hs.nshell <= 0 || hs.brute_shell.size() < (size_t)rt::kShellRecF) return false;
    const int32_t w = as_i32(hs.brute_shell[7]);
    hs.brute_shell[7] = as_f32(direct != 0 ? (w | rt::kShellDirect) : (w & ~rt::kShellDirect));
    return direct != 0;
}

bool materials_diffuse_only(const float* mat, int64_t nmat6) {
    // (int)t is 0 or 1 exactly for -1 < t < 2; a NaN type fails both comparisons
    for (int64_t m = 0; m < nmat6 / 6; ++m)
        if (!(mat[6 * m] > -1.0f && mat[6 * m] < 2.0f)) return false;
    return true;
}

void pack_checked(HostScene& hs, const float* bvh9, int64_t nb, int64_t ntri, int layout, int brute_max, int cluster,
                  int shell, int quad, std::string& why) {
    hs.fast_ok = (ntri > 0) ? pack_fast(hs, bvh9, nb, ntri, layout, brute_max, cluster, shell, quad, why) : true;
    if (hs.fast_ok && ntri > 0) {
        // the FAST kernels' Moller-Trumbore reciprocal (rt_device.h mt_recip) is IEEE-exact for
        // |a| <= 2^126, a = e1 . (d x e2) with |d| = 1: bound |e1| |e2| (finite edges; an infinite or
        // NaN edge makes a infinite or NaN, which mt_recip also returns exactly) 64x below it
        double m1 = 0.0, m2 = 0.0;
        for (int64_t t = 0; t < ntri; ++t) {
            const float* g = hs.tri_geo.data() + 12 * t;
            const double l1 = std::sqrt((double)g[4] * g[4] + (double)g[5] * g[5] + (double)g[6] * g[6]);
            const double l2 = std::sqrt((double)g[8] * g[8] + (double)g[9] * g[9] + (double)g[10] * g[10]);
            if (std::isfinite(l1)) m1 = std::max(m1, l1);
            if (std::isfinite(l2)) m2 = std::max(m2, l2);
        }
        if (!(m1 * m2 <= std::ldexp(1.0, 120))) {
            hs.fast_ok = false;
            why = "triangle edges beyond 2^60 (the FAST reciprocal needs |e1 . (d x e2)| <= 2^126)";
        }
    }
    if (ntri == 0) {
        hs.nnodes = 0; hs.root_ref = 0; hs.depth = 1; hs.nodes.clear();
        hs.nwnodes = 0; hs.wroot_ref = 0; hs.wdepth = 1; hs.wnodes.clear(); hs.wleaves.clear();
        hs.brute.clear(); hs.brute_box.clear(); hs.nbrute = 0; hs.nbox = 0;
    }
    if (!hs.fast_ok) { hs.brute.clear(); hs.brute_box.clear(); hs.nbrute = 0; hs.nbox = 0; }
    if (hs.nbrute == 0) { hs.brute_cbox.clear(); hs.brute_crow.clear(); hs.ncluster = 0; hs.nsingle = 0; hs.brute_near.clear(); }
    if (hs.ncluster == 0) { hs.brute_shell.clear(); hs.nshell = 0; hs.nrest = 0; hs.shell_floor = 0.0f; hs.shell_mask = 0; hs.nquad = 0; }
    if (!hs.fast_ok || hs.wdepth > 64) { hs.wnodes.clear(); hs.wleaves.clear(); hs.nwnodes = 0; hs.wdepth = 1; }
    // render kernels keep kStackLds entries in LDS and spill deeper ones to HBM; the single-ray
    // debug kernel keeps the whole stack in LDS (int2 entries, 128 lanes): depth <= 64
    if (hs.fast_ok && hs.depth > 64) {
        hs.fast_ok = false;
        why = "tree deeper than 64 levels";
    }
    if (hs.nodes.empty()) hs.nodes.assign(4 * rt::kNodeF4, 0.0f);
    if (hs.brute.empty()) hs.brute.assign(16, 0.0f);
    if (hs.brute_box.empty()) {   // never read (nbox = 0): one group of padding slots, ids valid all the same
        hs.brute_box.assign(8 * rt::kBoxGroup, 0.0f);
        for (int g = 0; g < rt::kBoxGroup; ++g) pad_box(hs.brute_box.data() + 8 * g);
    }
}

namespace {

int scene_prepare_(HostScene& hs, const float* vp, int64_t nvp, const float* vn, int64_t nvn, const int32_t* face,
                   int64_t nface, const float* mat, int64_t nmat, const float* bvh9, int64_t nbvh, int layout,
                   int brute_max, int cluster, int shell, int quad, std::string& msg, std::string& why) {
    if (nvp < 0 || nvp % 3 || nvn < 0 || nvn % 3 || nface < 0 || nface % 10 || nmat <= 0 || nmat % 6 || nbvh < 0 ||
        nbvh % 9)
        return fail(msg, RT_ERR_ARG,
                       "bad array sizes (V_p %lld, V_n %lld, faceData %lld, materialData %lld, BVH %lld)",
                       (long long)nvp, (long long)nvn, (long long)nface, (long long)nmat, (long long)nbvh);
    if ((nface && (!vp || !vn || !face)) || !mat || (nbvh && !bvh9))
        return fail(msg, RT_ERR_ARG, "null array");
    const int64_t T = nface / 10, NV = nvp / 3, NN = nvn / 3, M = nmat / 6, NB = nbvh / 9;
    if (T > 0x3fffffff || NB > 0x7fffffff) return fail(msg, RT_ERR_ARG, "scene too large");
    if (T > 0 && NB == 0) return fail(msg, RT_ERR_SCENE, "triangles given without a BVH");
    for (int64_t m = 0; m < M; ++m) {
        const float tf = mat[6 * m];
        if (!(tf > -1.0f && tf < 4.0f))
            return fail(msg, RT_ERR_SCENE, "material %lld has type %g; the kernel defines types 0..3", (long long)m,
                           (double)tf);
    }
    hs.ntri = (int32_t)T;
    hs.nmat = (int32_t)M;
    hs.nbvh9 = (int32_t)NB;
    hs.mat.assign((size_t)rt::kMatF * M, 0.0f);   // rows padded to kMatF floats (DevScene::mat)
    for (int64_t m = 0; m < M; ++m) {
        for (int k = 0; k < 6; ++k) hs.mat[(size_t)rt::kMatF * m + k] = mat[6 * m + k];
        for (int k = 1; k < 4; ++k) hs.colors_finite = hs.colors_finite && std::isfinite(mat[6 * m + k]);
        hs.has_glass = hs.has_glass || (int)mat[6 * m] == 3;
    }
    hs.diffuse_only = materials_diffuse_only(mat, nmat);
    if (bvh9) hs.bvh9.assign(bvh9, bvh9 + nbvh);
    hs.tri_geo.assign((size_t)T * 12, 0.0f);
    hs.tri_shade.assign((size_t)T * 4, 0.0f);
    for (int64_t t = 0; t < T; ++t) {
        const int32_t* f = face + 10 * t;
        if (f[0] < 0 || f[0] >= M)
            return fail(msg, RT_ERR_ARG, "triangle %lld: material %d out of range [0,%lld)", (long long)t, f[0],
                           (long long)M);
        for (int j = 7; j < 10; ++j)
            if (f[j] < 0 || f[j] >= NV)
                return fail(msg, RT_ERR_ARG, "triangle %lld: position index %d out of range", (long long)t, f[j]);
        if (f[4] < 0 || f[4] >= NN)
            return fail(msg, RT_ERR_ARG, "triangle %lld: normal index %d out of range", (long long)t, f[4]);
        const float* a = vp + 3 * (int64_t)f[7];
        const float* b = vp + 3 * (int64_t)f[8];
        const float* c = vp + 3 * (int64_t)f[9];
        float* g = hs.tri_geo.data() + 12 * t;
        g[0] = a[0]; g[1] = a[1]; g[2] = a[2]; g[3] = 0.0f;
        g[4] = b[0] - a[0]; g[5] = b[1] - a[1]; g[6] = b[2] - a[2]; g[7] = 0.0f;
        g[8] = c[0] - a[0]; g[9] = c[1] - a[1]; g[10] = c[2] - a[2]; g[11] = 0.0f;
        const float* n = vn + 3 * (int64_t)f[4];
        float* sh = hs.tri_shade.data() + 4 * t;
        sh[0] = n[0]; sh[1] = n[1]; sh[2] = n[2]; sh[3] = as_f32(f[0]);
    }
    // REF traversal safety: every index the reference would follow must be in range.
    for (int64_t i = 0; i < NB; ++i) {
        int32_t l, r, t;
        if (!fidx(bvh9[9 * i + 0], NB, &l) || !fidx(bvh9[9 * i + 1], NB, &r) || !fidx(bvh9[9 * i + 8], T, &t))
            return fail(msg, RT_ERR_SCENE, "BVH node %lld has an index out of range", (long long)i);
    }
    // The reference loops forever on a cyclic node graph; refuse it instead of hanging the GPU.
    if (NB > 0) {
        std::vector<uint8_t> color(NB, 0);  // 0 new, 1 on path, 2 done
        std::vector<std::pair<int32_t, int>> st;
        st.push_back({0, 0});
        color[0] = 1;
        while (!st.empty()) {
            auto& top = st.back();
            const int32_t n = top.first;
            if (top.second < 2) {
                const int32_t ch = (int32_t)bvh9[9 * (int64_t)n + top.second];
                ++top.second;
                if (ch < 0) continue;
                if (color[ch] == 1) return fail(msg, RT_ERR_SCENE, "BVH node graph has a cycle through node %d", ch);
                if (color[ch] == 0) { color[ch] = 1; st.push_back({ch, 0}); }
            } else {
                color[n] = 2;
                st.pop_back();
            }
        }
    }
    pack_checked(hs, bvh9, NB, T, layout, brute_max, cluster, shell, quad, why);
    return RT_OK;
}

}  // namespace

// No C++ exception leaves the C ABI: a scene too large for host memory is an error status.
int scene_prepare(HostScene& hs, const float* vp, int64_t nvp, const float* vn, int64_t nvn, const int32_t* face,
                  int64_t nface, const float* mat, int64_t nmat, const float* bvh9, int64_t nbvh, int layout,
                  int brute_max, int cluster, int shell, int quad, std::string& msg, std::string& why) {
    try {
        return scene_prepare_(hs, vp, nvp, vn, nvn, face, nface, mat, nmat, bvh9, nbvh, layout, brute_max, cluster, shell,
                              quad, msg, why);
    } catch (const std::bad_alloc&) {
        hs = HostScene();
        return fail(msg, RT_ERR_ARG, "scene too large for host memory");
    } catch (const std::exception& e) {
        hs = HostScene();
        return fail(msg, RT_ERR_ARG, "scene preparation failed: %s", e.what());
    }
}

}  // namespace rt

namespace {
thread_local std::string g_check_error;
}

extern "C" int rt_scene_check(const float* vp, int64_t nvp, const float* vn, int64_t nvn, const int32_t* face,
                              int64_t nface, const float* mat, int64_t nmat, const float* bvh9, int64_t nbvh,
                              int layout, int64_t info[8]) {
    HostScene hs;
    std::string msg, why;
    if (layout != RT_BVH_REFERENCE && layout != RT_BVH_SAH) {
        g_check_error = "layout must be RT_BVH_REFERENCE or RT_BVH_SAH";
        return RT_ERR_ARG;
    }
    const int rc = rt::scene_prepare(hs, vp, nvp, vn, nvn, face, nface, mat, nmat, bvh9, nbvh, layout,
                                     RT_BRUTE_MAX_DEFAULT, -1, -1, -1, msg, why);
    g_check_error = rc != RT_OK ? msg : hs.fast_ok ? std::string() : "FAST traversal unavailable (" + why + ")";
    if (rc == RT_OK && info) {
        info[0] = hs.ntri;
        info[1] = hs.nnodes;
        info[2] = hs.depth;
        info[3] = hs.nwnodes;
        info[4] = hs.wdepth;
        info[5] = hs.nbrute;
        info[6] = hs.nbox;
        info[7] = hs.fast_ok ? 1 : 0;
    }
    return rc;
}

extern "C" const char* rt_scene_last_error(void) { return g_check_error.c_str(); }

extern "C" int rt_debug_brute_layout(const float* vp, int64_t nvp, const float* vn, int64_t nvn, const int32_t* face,
                                     int64_t nface, const float* mat, int64_t nmat, const float* bvh9, int64_t nbvh,
                                     int layout, float* boxes, int64_t cap, int64_t info[3]) {
    HostScene hs;
    std::string msg, why;
    if (layout != RT_BVH_REFERENCE && layout != RT_BVH_SAH) {
        g_check_error = "layout must be RT_BVH_REFERENCE or RT_BVH_SAH";
        return RT_ERR_ARG;
    }
    if (!info || cap < 0 || (cap > 0 && !boxes)) {
        g_check_error = "null info, or a box capacity without an array";
        return RT_ERR_ARG;
    }
    const int rc = rt::scene_prepare(hs, vp, nvp, vn, nvn, face, nface, mat, nmat, bvh9, nbvh, layout,
                                     RT_BRUTE_MAX_DEFAULT, -1, -1, -1, msg, why);
    g_check_error = rc != RT_OK ? msg : hs.fast_ok ? std::string() : "FAST traversal unavailable (" + why + ")";
    if (rc != RT_OK) return rc;
    info[0] = hs.nbox;
    info[1] = hs.nbrute;
    info[2] = (int64_t)hs.brute_box.size();
    const int64_t n = std::min<int64_t>(cap, info[2]);
    if (n > 0) std::memcpy(boxes, hs.brute_box.data(), (size_t)n * sizeof(float));
    return RT_OK;
}

extern "C" int rt_debug_brute_clusters(const float* vp, int64_t nvp, const float* vn, int64_t nvn, const int32_t* face,
                                       int64_t nface, const float* mat, int64_t nmat, const float* bvh9, int64_t nbvh,
                                       int layout, int cluster, float* slots, int64_t slot_cap, float* rows,
                                       int64_t row_cap, int64_t info[4]) {
    HostScene hs;
    std::string msg, why;
    if (layout != RT_BVH_REFERENCE && layout != RT_BVH_SAH) {
        g_check_error = "layout must be RT_BVH_REFERENCE or RT_BVH_SAH";
        return RT_ERR_ARG;
    }
    if (cluster < -1 || cluster > 1) {
        g_check_error = "brute_cluster must be -1 (auto), 0 (off) or 1 (force)";
        return RT_ERR_ARG;
    }
    if (!info || slot_cap < 0 || row_cap < 0 || (slot_cap > 0 && !slots) || (row_cap > 0 && !rows)) {
        g_check_error = "null info, or a capacity without an array";
        return RT_ERR_ARG;
    }
    const int rc = rt::scene_prepare(hs, vp, nvp, vn, nvn, face, nface, mat, nmat, bvh9, nbvh, layout,
                                     RT_BRUTE_MAX_DEFAULT, cluster, -1, -1, msg, why);
    g_check_error = rc != RT_OK ? msg : hs.fast_ok ? std::string() : "FAST traversal unavailable (" + why + ")";
    if (rc != RT_OK) return rc;
    info[0] = hs.ncluster;
    info[1] = hs.nsingle;
    info[2] = (int64_t)hs.brute_cbox.size();
    info[3] = (int64_t)hs.brute_crow.size();
    const int64_t ns = std::min<int64_t>(slot_cap, info[2]), nr = std::min<int64_t>(row_cap, info[3]);
    if (ns > 0) std::memcpy(slots, hs.brute_cbox.data(), (size_t)ns * sizeof(float));
    if (nr > 0) std::memcpy(rows, hs.brute_crow.data(), (size_t)nr * sizeof(float));
    return RT_OK;
}

extern "C" int rt_debug_brute_shell(const float* vp, int64_t nvp, const float* vn, int64_t nvn, const int32_t* face,
                                    int64_t nface, const float* mat, int64_t nmat, const float* bvh9, int64_t nbvh,
                                    int layout, int cluster, int shell, float* rec, int64_t cap, int64_t info[3]) {
    HostScene hs;
    std::string msg, why;
    if (layout != RT_BVH_REFERENCE && layout != RT_BVH_SAH) {
        g_check_error = "layout must be RT_BVH_REFERENCE or RT_BVH_SAH";
        return RT_ERR_ARG;
    }
    if (cluster < -1 || cluster > 1 || shell < -1 || shell > 1) {
        g_check_error = "brute_cluster and brute_shell must be -1 (auto), 0 (off) or 1 (force)";
        return RT_ERR_ARG;
    }
    if (!info || cap < 0 || (cap > 0 && !rec)) {
        g_check_error = "null info, or a capacity without an array";
        return RT_ERR_ARG;
    }
    const int rc = rt::scene_prepare(hs, vp, nvp, vn, nvn, face, nface, mat, nmat, bvh9, nbvh, layout,
                                     RT_BRUTE_MAX_DEFAULT, cluster, shell, -1, msg, why);
    g_check_error = rc != RT_OK ? msg : hs.fast_ok ? std::string() : "FAST traversal unavailable (" + why + ")";
    if (rc != RT_OK) return rc;
    info[0] = hs.nshell;
    info[1] = hs.nrest;
    info[2] = (int64_t)hs.brute_shell.size();
    const int64_t n = std::min<int64_t>(cap, info[2]);
    if (n > 0) std::memcpy(rec, hs.brute_shell.data(), (size_t)n * sizeof(float));
    return RT_OK;
}

extern "C" int rt_debug_brute_near(const float* vp, int64_t nvp, const float* vn, int64_t nvn, const int32_t* face,
                                   int64_t nface, const float* mat, int64_t nmat, const float* bvh9, int64_t nbvh,
                                   int layout, int cluster, int shell, int32_t* flags, int64_t cap, float* floor,
                                   int64_t info[2]) {
    HostScene hs;
    std::string msg, why;
    if (layout != RT_BVH_REFERENCE && layout != RT_BVH_SAH) {
        g_check_error = "layout must be RT_BVH_REFERENCE or RT_BVH_SAH";
        return RT_ERR_ARG;
    }
    if (cluster < -1 || cluster > 1 || shell < -1 || shell > 1) {
        g_check_error = "brute_cluster and brute_shell must be -1 (auto), 0 (off) or 1 (force)";
        return RT_ERR_ARG;
    }
    if (!info || !floor || cap < 0 || (cap > 0 && !flags)) {
        g_check_error = "null info or floor, or a capacity without an array";
        return RT_ERR_ARG;
    }
    const int rc = rt::scene_prepare(hs, vp, nvp, vn, nvn, face, nface, mat, nmat, bvh9, nbvh, layout,
                                     RT_BRUTE_MAX_DEFAULT, cluster, shell, -1, msg, why);
    g_check_error = rc != RT_OK ? msg : hs.fast_ok ? std::string() : "FAST traversal unavailable (" + why + ")";
    if (rc != RT_OK) return rc;
    info[0] = (int64_t)hs.brute_near.size();
    info[1] = hs.nshell;
    *floor = hs.shell_floor;
    const int64_t n = std::min<int64_t>(cap, info[0]);
    for (int64_t g = 0; g < n; ++g) flags[g] = hs.brute_near[(size_t)g];
    return RT_OK;
}

extern "C" int rt_debug_brute_direct(const float* vp, int64_t nvp, const float* vn, int64_t nvn, const int32_t* face,
                                     int64_t nface, const float* mat, int64_t nmat, const float* bvh9, int64_t nbvh,
                                     int layout, int cluster, int shell, int direct, int64_t info[3]) {
    HostScene hs;
    std::string msg, why;
    if (layout != RT_BVH_REFERENCE && layout != RT_BVH_SAH) {
        g_check_error = "layout must be RT_BVH_REFERENCE or RT_BVH_SAH";
        return RT_ERR_ARG;
    }
    if (cluster < -1 || cluster > 1 || shell < -1 || shell > 1) {
        g_check_error = "brute_cluster and brute_shell must be -1 (auto), 0 (off) or 1 (force)";
        return RT_ERR_ARG;
    }
    if (direct < -1 || direct > 1) {
        g_check_error = "brute_direct must be -1 (auto), 0 (off) or 1 (auto)";
        return RT_ERR_ARG;
    }
    if (!info) {
        g_check_error = "null info";
        return RT_ERR_ARG;
    }
    const int rc = rt::scene_prepare(hs, vp, nvp, vn, nvn, face, nface, mat, nmat, bvh9, nbvh, layout,
                                     RT_BRUTE_MAX_DEFAULT, cluster, shell, -1, msg, why);
    g_check_error = rc != RT_OK ? msg : hs.fast_ok ? std::string() : "FAST traversal unavailable (" + why + ")";
    if (rc != RT_OK) return rc;
    info[1] = rt::shell_direct(hs, direct) ? 1 : 0;
    info[0] = hs.nshell;
    info[2] = hs.nshell > 0 ? (int64_t)as_i32(hs.brute_shell[7]) : 0;
    return RT_OK;
}

extern "C" int rt_debug_brute_quad(const float* vp, int64_t nvp, const float* vn, int64_t nvn, const int32_t* face,
                                   int64_t nface, const float* mat, int64_t nmat, const float* bvh9, int64_t nbvh,
                                   int layout, int cluster, int shell, int quad, int32_t flags[6], float lines[24],
                                   int32_t words[18], float recs[108], float guard[3], int64_t info[2]) {
    HostScene hs;
    std::string msg, why;
    if (layout != RT_BVH_REFERENCE && layout != RT_BVH_SAH) {
        g_check_error = "layout must be RT_BVH_REFERENCE or RT_BVH_SAH";
        return RT_ERR_ARG;
    }
    if (cluster < -1 || cluster > 1 || shell < -1 || shell > 1) {
        g_check_error = "brute_cluster and brute_shell must be -1 (auto), 0 (off) or 1 (force)";
        return RT_ERR_ARG;
    }
    if (quad < -1 || quad > 1) {
        g_check_error = "brute_quad must be -1 (auto), 0 (off) or 1 (auto)";
        return RT_ERR_ARG;
    }
    if (!info || !flags || !lines || !words || !recs || !guard) {
        g_check_error = "null info, flags, lines, words, recs or guard";
        return RT_ERR_ARG;
    }
    const int rc = rt::scene_prepare(hs, vp, nvp, vn, nvn, face, nface, mat, nmat, bvh9, nbvh, layout,
                                     RT_BRUTE_MAX_DEFAULT, cluster, shell, quad, msg, why);
    g_check_error = rc != RT_OK ? msg : hs.fast_ok ? std::string() : "FAST traversal unavailable (" + why + ")";
    if (rc != RT_OK) return rc;
    info[0] = hs.nshell;
    info[1] = hs.nquad;
    guard[0] = rt::kQuadBand; guard[1] = rt::kQuadGraze; guard[2] = rt::kQuadDirMax;
    for (int f = 0; f < 6; ++f) {
        flags[f] = 0;
        for (int k = 0; k < 4; ++k) lines[4 * f + k] = 0.0f;
        for (int k = 0; k < 3; ++k) words[3 * f + k] = -1;
        for (int k = 0; k < 18; ++k) recs[18 * f + k] = 0.0f;
        if (hs.nshell == 0) continue;
        const float* row = hs.brute_shell.data() + 4 * rt::kShellRowF4 + 8 * f;
        std::memcpy(lines + 4 * f, row, 16);
        std::memcpy(words + 3 * f, row + 4, 12);
        std::memcpy(flags + f, row + 7, 4);
        // the records as Moller-Trumbore reads them: p0, e1, e2 of the first, then of the second
        const uint32_t both = (uint32_t)words[3 * f];
        for (int j = 0; j < 2; ++j) {
            const uint32_t q = j ? both >> 16 : both & 0xffffu;
            if (both != ~0u && q != 0xffffu && (int32_t)q < hs.nbrute)
                std::memcpy(recs + 18 * f + 9 * j, hs.brute.data() + 16 * (size_t)q + 6, 9 * sizeof(float));
        }
    }
    return RT_OK;
}

// rt_reproject_basis (rt_api.h): the previous camera as the reprojection kernel takes it -- genCameraRay's three
// rotations undone on the unit vectors, the position, the focal length as make_const (rt_device.h) has it, the width.
// Host only: rtm.h gives the bits the launch constants have.
extern "C" int rt_reproject_basis(const float cam[10], float basis[16]) {
    if (!cam || !basis) return RT_ERR_ARG;
    for (int k = 0; k < 10; ++k)
        if (!std::isfinite(cam[k])) return RT_ERR_ARG;
    for (int j = 0; j < 3; ++j) {
        rtm_f3 e = rtm_v3(j == 0 ? 1.0f : 0.0f, j == 1 ? 1.0f : 0.0f, j == 2 ? 1.0f : 0.0f);
        e = rtm_rotate(-(cam[5] * (3.14f / 180.0f)), rtm_v3(0, 0, 1), e);
        e = rtm_rotate(-(cam[4] * (3.14f / 180.0f)), rtm_v3(0, 1, 0), e);
        e = rtm_rotate(-(cam[3] * (3.14f / 180.0f)), rtm_v3(1, 0, 0), e);
        basis[j] = e.x;
        basis[3 + j] = e.y;
        basis[6 + j] = e.z;
    }
    basis[9] = cam[0];
    basis[10] = cam[1];
    basis[11] = cam[2];
    const float focal_y = cam[1] - (1.0f / (2.0f * rtm_tan(cam[9] / 2.0f)));
    basis[12] = cam[1] - focal_y;
    basis[13] = cam[6];
    basis[14] = 0.0f;
    basis[15] = 0.0f;
    return RT_OK;
}
