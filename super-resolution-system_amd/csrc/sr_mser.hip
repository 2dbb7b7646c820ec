// sr_mser.hip -- MSER text regions (ContentAnalyzer.detect_text_regions, tiling_module.py:214-237) on gfx950: the component
// tree of the gray plane by a level-synchronous union-find, then the selection rules of include/sr_hip.h ("MSER"), one
// thread per node.  Every quantity is an integer and every atomic an integer atomic: the tree is a property of the image,
// so equal inputs give equal records whatever order the hardware takes.
//
//   k_ms_gray      gray plane (the content section's gray_swapped; 255 - g for the bright polarity) + 256-bin histogram
//                  (counted per block in LDS, one global add per non-empty bin and block)
//   (host)         the 256 counts come down once: empty levels launch nothing; their prefix sums go back as cursors
//   k_ms_scatter   pixel indices by level: rank inside the block from LDS, one global add per non-empty bin and block
//   per non-empty level t, over the pixels L_t of that level:
//   k_ms_note      parent[p] = p; for every neighbour below t: its root r (compressing the neighbour's path); the first
//                  thread to take r's node id out of node_of_root[r] (atomicExch) appends (r, node) to the level's list --
//                  the old roots that touch the level, with their nodes, deduplicated, before any union
//   k_ms_union     union(p, q) for every neighbour q with g(q) <= t (same-level edges from their smaller end)
//   k_ms_create    parent[p] = root(p); the first thread to claim a changed root R (node_of_root[R]: -1 -> id, by CAS)
//                  creates its node {t, area 0, empty box, seed R}
//   k_ms_accum     the level's pixels add 1 and their position, the listed old nodes add their area and box, into the node
//                  of their root; the old nodes get that node as parent.  Lanes of a wave that share a node are reduced by
//                  shuffles and add once: a flat image sends every pixel to one node, and one word takes ~88 M atomics/s
//   k_ms_S / k_ms_edges / k_ms_filter / k_ms_pick   S by at most delta parent steps; every edge stores 0 into the flag of
//                  the end with the larger variation (int64 cross-multiplication; racing stores of one value); the
//                  filters; the diversity walk against the nearest passing ancestor and a compaction of the kept indices
//   k_ms_records   the kept nodes as records; the host sorts them (polarity, level, seed)
//
// The root of a set is its SMALLEST pixel index, so `seed` is the root and no result depends on the order of the unions.
//
// Coherence (MI355X: per-XCD L2s are not coherent with each other, a CU's L1 is never refreshed by another CU's stores).
// k_ms_union is the only kernel in which parents change while they are read, and there correctness rests on (1) alone:
//   (1) by construction: parent[x] only ever decreases (CAS on a root installs a smaller index, atomicMin shortens a path
//       to an ancestor), and a word that once named a smaller index never names x again.  A stale parent is therefore an
//       earlier value: x itself or a former ancestor, in either case a member of x's set.  A find that ends on a stale
//       "root" a is corrected by the CAS on parent[a], which is performed at the memory side: it fails with the current
//       parent and the walk goes on from there; linking under a b that has meanwhile stopped being a root is still a link
//       to a smaller member of the right set.  a == b from stale reads is still a true statement of membership.
//   (2) the loads of find in that kernel are __hip_atomic_load(relaxed, agent) all the same.  They bypass the CU's L1 only
//       and are served from the XCD's own L2, which another XCD's unions do not refresh: they are no guarantee, they only
//       shorten the walks over what this XCD's CUs have linked meanwhile.
// ACROSS kernels the design relies on the kernel boundary, and on nothing else, for visibility through L2: node_of_root[]
// and parent[] are changed by atomics and plain stores in one kernel and read through L1 / L2 in the next; every other kernel
// reads words that the previous kernel finished writing, or that racing writers of its own set to one and the same value
// (path compression towards a root that does not change in that kernel; the agent-scope loads before the claim atomics of
// k_ms_note / k_ms_create only spare attempts, the atomic decides).  A persistent kernel over the levels would lose that
// boundary and needs agent-scope release / acquire between its phases: this argument does not carry over to it.
//
// Between the histogram download and the download of the region count there is no host synchronisation: the length of a
// level's list and the node count stay on the device; launches are sized to a bound and blocks past the count leave.
#include <algorithm>
#include <climits>
#include <vector>

#include "sr_ctx.h"
#include "sr_mser.h"

namespace {

#define MS_THREADS 256
#define MS_CHUNK 4096            // pixels per block of the histogram and the scatter (16 per thread)
#define MS_MAXGRID 8192
#define MS_CTR_CURSOR 256
#define MS_CTR_LIST 512
#define MS_CTR_NODES 768
#define MS_CTR_REGIONS 769

__device__ __forceinline__ int ms_gray(const unsigned char *px, int cn)
{
    return cn == 1 ? px[0] : (px[0] * 3735 + px[1] * 19235 + px[2] * 9798 + (1 << 14)) >> 15;
}

__global__ __launch_bounds__(MS_THREADS) void k_ms_gray(const unsigned char *__restrict__ img, long long stride, int cn, int H,
                                                        int W, int bright, unsigned char *__restrict__ g,
                                                        unsigned *__restrict__ hist)
{
    __shared__ unsigned cnt[256];
    const int N = H * W;
    cnt[threadIdx.x] = 0u;
    __syncthreads();
    const int base = blockIdx.x * MS_CHUNK;
    for (int i = threadIdx.x; i < MS_CHUNK; i += MS_THREADS) {
        const int p = base + i;
        if (p < N) {
            const int y = p / W, x = p - y * W;
            int v = ms_gray(img + (long long)y * stride + (long long)x * cn, cn);
            if (bright) v = 255 - v;
            g[p] = (unsigned char)v;
            atomicAdd(&cnt[v], 1u);
        }
    }
    __syncthreads();
    if (cnt[threadIdx.x]) atomicAdd(&hist[threadIdx.x], cnt[threadIdx.x]);
}

__global__ __launch_bounds__(MS_THREADS) void k_ms_scatter(const unsigned char *__restrict__ g, int N, unsigned *__restrict__ cursor,
                                                           int *__restrict__ order)
{
    __shared__ unsigned cnt[256], start[256];
    cnt[threadIdx.x] = 0u;
    __syncthreads();
    const int base = blockIdx.x * MS_CHUNK;
    unsigned rank[MS_CHUNK / MS_THREADS];
    int val[MS_CHUNK / MS_THREADS];
#pragma unroll
    for (int k = 0; k < MS_CHUNK / MS_THREADS; ++k) {
        const int p = base + k * MS_THREADS + threadIdx.x;
        val[k] = p < N ? (int)g[p] : -1;
        rank[k] = val[k] >= 0 ? atomicAdd(&cnt[val[k]], 1u) : 0u;
    }
    __syncthreads();
    if (cnt[threadIdx.x]) start[threadIdx.x] = atomicAdd(&cursor[threadIdx.x], cnt[threadIdx.x]);
    __syncthreads();
#pragma unroll
    for (int k = 0; k < MS_CHUNK / MS_THREADS; ++k) {
        const unsigned pos = val[k] >= 0 ? start[val[k]] + rank[k] : 0u;
        if (val[k] >= 0 && pos < (unsigned)N) order[pos] = base + k * MS_THREADS + threadIdx.x;
    }
}

// neighbour k of (y, x): up, down, left, right; -1 outside the image
__device__ __forceinline__ int ms_nbr(int p, int y, int x, int H, int W, int k)
{
    if (k == 0) return y > 0 ? p - W : -1;
    if (k == 1) return y + 1 < H ? p + W : -1;
    if (k == 2) return x > 0 ? p - 1 : -1;
    return x + 1 < W ? p + 1 : -1;
}

__device__ __forceinline__ int ms_find_plain(const int *parent, int p)
{
    int q;
    while ((q = parent[p]) != p) p = q;
    return p;
}

__device__ __forceinline__ int ms_find_atomic(int *parent, int p)
{
    int q = __hip_atomic_load(&parent[p], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    while (q != p) {
        const int gq = __hip_atomic_load(&parent[q], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (gq != q) atomicMin(&parent[p], gq);          // path halving: an ancestor, and smaller
        p = q;
        q = gq;
    }
    return p;
}

// One lane per distinct key among the lanes that need it: a flat zone sends a whole wave to one root, and the word behind it
// should see one atomic per wave, not sixty-four.
__device__ __forceinline__ bool ms_elect(bool need, int key)
{
    const int lane = threadIdx.x & 63;
    unsigned long long todo = __ballot(need);
    bool lead = false;
    while (todo) {
        const int src = __ffsll((long long)todo) - 1;
        const int k = __shfl(key, src);
        if (lane == src) lead = true;
        todo &= ~__ballot(need && key == k);
    }
    return lead;
}

__global__ __launch_bounds__(MS_THREADS) void k_ms_note(const unsigned char *__restrict__ g, int H, int W, int t,
                                                        const int *__restrict__ L, int nL, int *parent, int *nor, int2 *list,
                                                        int list_cap, unsigned *len)
{
    const int lane = threadIdx.x & 63;
    for (int base = blockIdx.x * MS_THREADS; base < nL; base += gridDim.x * MS_THREADS) {
        const int i = base + threadIdx.x;
        const bool valid = i < nL;
        int p = 0, y = 0, x = 0;
        if (valid) {
            p = L[i];
            y = p / W;
            x = p - y * W;
            parent[p] = p;
            nor[p] = -1;
        }
        for (int k = 0; k < 4; ++k) {
            int r = -1, nd = -1;
            const int q = valid ? ms_nbr(p, y, x, H, W, k) : -1;
            if (q >= 0 && (int)g[q] < t) {
                r = ms_find_plain(parent, q);
                if (r != q) parent[q] = r;               // every writer of this kernel stores this same root
            }
            // a node id leaves node_of_root[r] once: the load (agent scope: not an L1 copy from before the first taker)
            // spares the word most of the attempts, the election the rest
            const bool need = r >= 0 && __hip_atomic_load(&nor[r], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= 0;
            if (ms_elect(need, r)) nd = atomicExch(&nor[r], -1);
            // the winners of this wave take consecutive list slots with one add
            const unsigned long long win = __ballot(nd >= 0);
            if (win) {
                unsigned slot = 0;
                if (lane == __ffsll((long long)win) - 1) slot = atomicAdd(len, (unsigned)__popcll(win));
                slot = __shfl(slot, __ffsll((long long)win) - 1) + (unsigned)__popcll(win & ((1ULL << lane) - 1ULL));
                if (nd >= 0 && slot < (unsigned)list_cap) list[slot] = make_int2(r, nd);
            }
        }
    }
}

__device__ __forceinline__ void ms_unite(int *parent, int a, int b)
{
    a = ms_find_atomic(parent, a);
    b = ms_find_atomic(parent, b);
    while (a != b) {
        if (a < b) {
            const int s = a;
            a = b;
            b = s;
        }
        const int old = atomicCAS(&parent[a], a, b);     // the larger root goes under the smaller index
        if (old == a) break;
        a = ms_find_atomic(parent, old);
        b = ms_find_atomic(parent, b);
    }
}

__global__ __launch_bounds__(MS_THREADS) void k_ms_union(const unsigned char *__restrict__ g, int H, int W, int t,
                                                         const int *__restrict__ L, int nL, int *parent)
{
    for (int i = blockIdx.x * MS_THREADS + threadIdx.x; i < nL; i += gridDim.x * MS_THREADS) {
        const int p = L[i], y = p / W, x = p - y * W;
        for (int k = 0; k < 4; ++k) {
            const int q = ms_nbr(p, y, x, H, W, k);
            if (q < 0) continue;
            const int gq = g[q];
            if (gq < t || (gq == t && q > p)) ms_unite(parent, p, q);
        }
    }
}

__global__ __launch_bounds__(MS_THREADS) void k_ms_create(int t, const int *__restrict__ L, int nL, int *parent, int *nor,
                                                          MserNode *nodes, int node_cap, unsigned *node_count)
{
    const int lane = threadIdx.x & 63;
    for (int base = blockIdx.x * MS_THREADS; base < nL; base += gridDim.x * MS_THREADS) {
        const int i = base + threadIdx.x;
        int R = -1;
        bool need = false;
        if (i < nL) {
            const int p = L[i];
            R = ms_find_plain(parent, p);
            if (R != p) parent[p] = R;                   // the unions are over: every writer stores this same root
            need = __hip_atomic_load(&nor[R], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == -1;
        }
        const bool won = ms_elect(need, R) && atomicCAS(&nor[R], -1, -2) == -1;
        const unsigned long long win = __ballot(won);
        if (win) {
            unsigned id = 0;
            if (lane == __ffsll((long long)win) - 1) id = atomicAdd(node_count, (unsigned)__popcll(win));
            id = __shfl(id, __ffsll((long long)win) - 1) + (unsigned)__popcll(win & ((1ULL << lane) - 1ULL));
            if (won && id < (unsigned)node_cap) {
                nodes[id] = {t, 0, INT_MAX, INT_MAX, -1, -1, R, -1};
                __hip_atomic_store(&nor[R], (int)id, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
    }
}

// Adds (area, box) into nodes[id] for the valid lanes; lanes of the wave that share an id are reduced first.
__device__ __forceinline__ void ms_add(MserNode *nodes, bool valid, int id, int area, int x0, int y0, int x1, int y1)
{
    const int lane = threadIdx.x & 63;
    unsigned long long todo = __ballot(valid);
    while (todo) {
        const int src = __ffsll((long long)todo) - 1;
        const int k = __shfl(id, src);
        const bool mine = valid && id == k;
        const unsigned long long m = __ballot(mine);
        int a = mine ? area : 0, bx0 = mine ? x0 : INT_MAX, by0 = mine ? y0 : INT_MAX, bx1 = mine ? x1 : -1, by1 = mine ? y1 : -1;
        if (__popcll(m) > 1) {
            for (int o = 32; o > 0; o >>= 1) {
                a += __shfl_xor(a, o);
                bx0 = min(bx0, __shfl_xor(bx0, o));
                by0 = min(by0, __shfl_xor(by0, o));
                bx1 = max(bx1, __shfl_xor(bx1, o));
                by1 = max(by1, __shfl_xor(by1, o));
            }
        }
        if (lane == src) {
            MserNode *n = nodes + k;
            atomicAdd(&n->area, a);
            atomicMin(&n->x0, bx0);
            atomicMin(&n->y0, by0);
            atomicMax(&n->x1, bx1);
            atomicMax(&n->y1, by1);
        }
        todo &= ~m;
    }
}

__global__ __launch_bounds__(MS_THREADS) void k_ms_accum(int W, const int *__restrict__ L, int nL, int *parent,
                                                         const int *__restrict__ nor, const int2 *__restrict__ list,
                                                         const unsigned *__restrict__ len, int list_cap, MserNode *nodes,
                                                         int node_cap)
{
    const int nlist = (int)min(*len, (unsigned)list_cap);
    const int total = nL + nlist;
    for (int base = blockIdx.x * MS_THREADS; base < total; base += gridDim.x * MS_THREADS) {
        const int i = base + threadIdx.x;
        bool valid = i < total;
        int id = -1, area = 0, x0 = 0, y0 = 0, x1 = 0, y1 = 0;
        if (valid && i < nL) {
            const int p = L[i];
            id = nor[parent[p]];                         // k_ms_create left parent[p] at the root
            y0 = y1 = p / W;
            x0 = x1 = p - y0 * W;
            area = 1;
        } else if (valid) {
            const int2 e = list[i - nL];
            const int R = ms_find_plain(parent, e.x);
            if (R != e.x) parent[e.x] = R;
            id = nor[R];
            const bool ok = id >= 0 && id < node_cap && e.y >= 0 && e.y < node_cap;
            if (ok) {
                MserNode *o = nodes + e.y;
                area = o->area;
                x0 = o->x0;
                y0 = o->y0;
                x1 = o->x1;
                y1 = o->y1;
                o->parent = id;
            }
        }
        valid = valid && id >= 0 && id < node_cap;
        ms_add(nodes, valid, id, area, x0, y0, x1, y1);
    }
}

// ---- selection ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(MS_THREADS) void k_ms_S(const MserNode *__restrict__ nodes, const unsigned *__restrict__ node_count,
                                                     int node_cap, int delta, int *__restrict__ S, unsigned char *__restrict__ stable)
{
    const int nn = (int)min(*node_count, (unsigned)node_cap);
    for (int i = blockIdx.x * MS_THREADS + threadIdx.x; i < nn; i += gridDim.x * MS_THREADS) {
        const int lim = nodes[i].level + delta;
        int a = i;
        for (int step = 0; step < 256; ++step) {
            const int q = nodes[a].parent;
            if (q < 0 || q >= nn || nodes[q].level > lim) break;
            a = q;
        }
        S[i] = nodes[a].area;
        stable[i] = 1;
    }
}

__global__ __launch_bounds__(MS_THREADS) void k_ms_edges(const MserNode *__restrict__ nodes, const unsigned *__restrict__ node_count,
                                                         int node_cap, const int *__restrict__ S, unsigned char *stable)
{
    const int nn = (int)min(*node_count, (unsigned)node_cap);
    for (int c = blockIdx.x * MS_THREADS + threadIdx.x; c < nn; c += gridDim.x * MS_THREADS) {
        const int q = nodes[c].parent;
        if (q < 0 || q >= nn) continue;
        const long long ac = nodes[c].area, aq = nodes[q].area;
        const long long vc = ((long long)S[c] - ac) * aq, vq = ((long long)S[q] - aq) * ac;
        if (vc > vq) stable[c] = 0;
        if (vq > vc) stable[q] = 0;
    }
}

__global__ __launch_bounds__(MS_THREADS) void k_ms_filter(const MserNode *__restrict__ nodes, const unsigned *__restrict__ node_count,
                                                          int node_cap, const int *__restrict__ S,
                                                          const unsigned char *__restrict__ stable, int min_area, int max_area,
                                                          double max_variation, unsigned char *__restrict__ passed)
{
    const int nn = (int)min(*node_count, (unsigned)node_cap);
    for (int i = blockIdx.x * MS_THREADS + threadIdx.x; i < nn; i += gridDim.x * MS_THREADS) {
        const int a = nodes[i].area;
        const double lim = __dmul_rn(max_variation, (double)a);
        passed[i] = stable[i] && a >= min_area && a <= max_area && (double)(S[i] - a) < lim;
    }
}

__global__ __launch_bounds__(MS_THREADS) void k_ms_pick(const MserNode *__restrict__ nodes, const unsigned *__restrict__ node_count,
                                                        int node_cap, const unsigned char *__restrict__ passed, double min_diversity,
                                                        int *__restrict__ kept, unsigned *region_count)
{
    const int nn = (int)min(*node_count, (unsigned)node_cap);
    for (int i = blockIdx.x * MS_THREADS + threadIdx.x; i < nn; i += gridDim.x * MS_THREADS) {
        if (!passed[i]) continue;
        int a = nodes[i].parent;
        for (int step = 0; step < 256 && a >= 0 && a < nn && !passed[a]; ++step) a = nodes[a].parent;
        if (a >= 0 && a < nn) {
            const int aa = nodes[a].area;
            if ((double)(aa - nodes[i].area) < __dmul_rn(min_diversity, (double)aa)) continue;
        }
        const unsigned k = atomicAdd(region_count, 1u);
        if (k < (unsigned)node_cap) kept[k] = i;
    }
}

__global__ __launch_bounds__(MS_THREADS) void k_ms_records(const MserNode *__restrict__ nodes, const int *__restrict__ S,
                                                           const int *__restrict__ kept, int first, int n, int polarity,
                                                           sr_mser_region *__restrict__ out)
{
    for (int j = blockIdx.x * MS_THREADS + threadIdx.x; j < n; j += gridDim.x * MS_THREADS) {
        const int i = kept[first + j];
        const MserNode nd = nodes[i];
        out[j] = {polarity, nd.level, nd.area, nd.x0, nd.y0, nd.x1, nd.y1, nd.seed, S[i]};
    }
}

// ---- host side ------------------------------------------------------------------------------------------------------------
unsigned ms_grid(long long n)
{
    return (unsigned)std::max(1LL, std::min((n + MS_THREADS - 1) / MS_THREADS, (long long)MS_MAXGRID));
}

bool bad_image(const void *d_img, int64_t stride, int h, int w, int cn)
{
    return !d_img || h < 1 || w < 1 || (cn != 1 && cn != 3 && cn != 4) || stride < (int64_t)w * cn;
}

struct MsView {
    unsigned char *g;
    int *order, *parent, *nor;
    int2 *list;
    MserNode *nodes;
    unsigned *ctr;
    int list_cap, node_cap;
};

// The tree of one polarity into the workspace; the node count stays on the device (ctr[MS_CTR_NODES]).  One host
// synchronisation: the histogram.
int build_tree(sr_ctx *ctx, const char *who, const uint8_t *d_img, int64_t stride, int h, int w, int cn, int polarity,
               const MserPlan &pl, MsView *view)
{
    SRCHK(ctx->mser_ws.reserve(ctx, who, pl.total));
    char *ws = ctx->mser_ws.as<char>();
    MsView v;
    v.g = (unsigned char *)(ws + pl.off_gray);
    v.order = (int *)(ws + pl.off_order);
    v.parent = (int *)(ws + pl.off_parent);
    v.nor = (int *)(ws + pl.off_nor);
    v.list = (int2 *)(ws + pl.off_list);
    v.nodes = (MserNode *)(ws + pl.off_nodes);
    v.ctr = (unsigned *)(ws + pl.off_ctr);
    v.list_cap = (int)std::min<size_t>(pl.list_bytes / sizeof(int2), (size_t)pl.npx);
    v.node_cap = (int)pl.node_cap;
    *view = v;
    const int N = (int)pl.npx;
    const unsigned chunks = (unsigned)((N + MS_CHUNK - 1) / MS_CHUNK);
    unsigned counts[256];
    {
        ProfScope ps(ctx, "ms_sort");
        HIPCHK(hipMemsetAsync(v.ctr, 0, 4096, ctx->stream));
        hipLaunchKernelGGL(k_ms_gray, dim3(chunks), dim3(MS_THREADS), 0, ctx->stream, d_img, (long long)stride, cn, h, w, polarity,
                           v.g, v.ctr);
        SRCHK(check_launch(who));
        HIPCHK(hipMemcpyAsync(counts, v.ctr, sizeof(counts), hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(stream_sync(ctx));
    }
    unsigned start[257];
    start[0] = 0;
    for (int t = 0; t < 256; ++t) start[t + 1] = start[t] + counts[t];
    if (start[256] != (unsigned)N) return sr_set_error(SR_ERR_HIP, "%s: the histogram does not add up to the image", who);
    {
        ProfScope ps(ctx, "ms_sort");
        HIPCHK(upload_small(ctx, v.ctr + MS_CTR_CURSOR, start, 256 * sizeof(unsigned)));
        hipLaunchKernelGGL(k_ms_scatter, dim3(chunks), dim3(MS_THREADS), 0, ctx->stream, (const unsigned char *)v.g, N,
                           v.ctr + MS_CTR_CURSOR, v.order);
    }
    for (int t = 0; t < 256; ++t) {
        const int nL = (int)counts[t];
        if (!nL) continue;
        const int *L = v.order + start[t];
        unsigned *len = v.ctr + MS_CTR_LIST + t;
        const long long bound = std::min<long long>(4LL * nL, (long long)start[t]);      // old roots a level can touch
        const dim3 grid(ms_grid(nL)), block(MS_THREADS);
        {
            ProfScope ps(ctx, "ms_note");
            hipLaunchKernelGGL(k_ms_note, grid, block, 0, ctx->stream, (const unsigned char *)v.g, h, w, t, L, nL, v.parent, v.nor,
                               v.list, v.list_cap, len);
        }
        {
            ProfScope ps(ctx, "ms_union");
            hipLaunchKernelGGL(k_ms_union, grid, block, 0, ctx->stream, (const unsigned char *)v.g, h, w, t, L, nL, v.parent);
        }
        {
            ProfScope ps(ctx, "ms_create");
            hipLaunchKernelGGL(k_ms_create, grid, block, 0, ctx->stream, t, L, nL, v.parent, v.nor, v.nodes, v.node_cap,
                               v.ctr + MS_CTR_NODES);
        }
        {
            ProfScope ps(ctx, "ms_accum");
            hipLaunchKernelGGL(k_ms_accum, dim3(ms_grid(nL + bound)), block, 0, ctx->stream, w, L, nL, v.parent, (const int *)v.nor,
                               (const int2 *)v.list, (const unsigned *)len, v.list_cap, v.nodes, v.node_cap);
        }
    }
    return check_launch(who);
}

}  // namespace

int sr_mser_u8(sr_ctx *ctx, const uint8_t *d_img, int64_t stride, int h, int w, int cn, const sr_mser_params *params,
               int polarity_mask, sr_mser_region *h_regions, int64_t cap, int64_t *count)
{
    CTX_ENTER(ctx);
    ctx->mser_last.clear();
    if (bad_image(d_img, stride, h, w, cn) || !count || cap < 0 || (cap > 0 && !h_regions) || polarity_mask < 1 || polarity_mask > 3)
        return sr_set_error(SR_ERR_INVALID_ARG, "sr_mser_u8: bad arguments");
    SRCHK(mser_check("sr_mser_u8", h, w, params));
    MserPlan pl;
    mser_layout(h, w, &pl);
    std::vector<sr_mser_region> all;
    for (int pol = 0; pol < 2; ++pol) {
        if (!(polarity_mask >> pol & 1)) continue;
        MsView v;
        SRCHK(build_tree(ctx, "sr_mser_u8", d_img, stride, h, w, cn, pol, pl, &v));
        // the sections of the build that are dead now carry the selection (sr_mser.h)
        int *S = v.order, *kept = v.parent;
        unsigned char *stable = (unsigned char *)v.nor, *passed = stable + pl.npx;
        const dim3 grid(ms_grid(pl.node_cap)), block(MS_THREADS);
        {
            ProfScope ps(ctx, "ms_select");
            hipLaunchKernelGGL(k_ms_S, grid, block, 0, ctx->stream, (const MserNode *)v.nodes, (const unsigned *)(v.ctr + MS_CTR_NODES),
                               v.node_cap, params->delta, S, stable);
            hipLaunchKernelGGL(k_ms_edges, grid, block, 0, ctx->stream, (const MserNode *)v.nodes,
                               (const unsigned *)(v.ctr + MS_CTR_NODES), v.node_cap, (const int *)S, stable);
            hipLaunchKernelGGL(k_ms_filter, grid, block, 0, ctx->stream, (const MserNode *)v.nodes,
                               (const unsigned *)(v.ctr + MS_CTR_NODES), v.node_cap, (const int *)S, (const unsigned char *)stable,
                               params->min_area, params->max_area, params->max_variation, passed);
            hipLaunchKernelGGL(k_ms_pick, grid, block, 0, ctx->stream, (const MserNode *)v.nodes,
                               (const unsigned *)(v.ctr + MS_CTR_NODES), v.node_cap, (const unsigned char *)passed,
                               params->min_diversity, kept, v.ctr + MS_CTR_REGIONS);
        }
        SRCHK(check_launch("sr_mser_u8"));
        unsigned tail[2] = {0, 0};                          // nodes, regions
        HIPCHK(hipMemcpyAsync(tail, v.ctr + MS_CTR_NODES, sizeof(tail), hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(stream_sync(ctx));
        if (tail[0] > (unsigned)v.node_cap || tail[1] > tail[0])
            return sr_set_error(SR_ERR_HIP, "sr_mser_u8: node table overflow (%u nodes, %u regions)", tail[0], tail[1]);
        const int nreg = (int)tail[1];
        const int chunk = (int)(pl.list_bytes / sizeof(sr_mser_region));
        sr_mser_region *d_rec = (sr_mser_region *)v.list;
        const size_t at = all.size();
        all.resize(at + nreg);
        for (int first = 0; first < nreg; first += chunk) {
            const int m = std::min(chunk, nreg - first);
            hipLaunchKernelGGL(k_ms_records, dim3(ms_grid(m)), block, 0, ctx->stream, (const MserNode *)v.nodes, (const int *)S,
                               (const int *)kept, first, m, pol, d_rec);
            SRCHK(check_launch("sr_mser_u8"));
            HIPCHK(hipMemcpyAsync(all.data() + at + first, d_rec, (size_t)m * sizeof(sr_mser_region), hipMemcpyDeviceToHost,
                                  ctx->stream));
            HIPCHK(stream_sync(ctx));
        }
    }
    mser_sort_regions(all.data(), all.size());
    *count = (int64_t)all.size();
    const size_t m = std::min<size_t>(all.size(), (size_t)cap);
    if (m) std::copy(all.begin(), all.begin() + m, h_regions);
    ctx->mser_last.swap(all);
    return SR_OK;
}

int sr_mser_last_regions(sr_ctx *ctx, sr_mser_region *h_regions, int64_t cap, int64_t *count)
{
    CTX_ENTER(ctx);
    if (!count || cap < 0 || (cap > 0 && !h_regions)) return sr_set_error(SR_ERR_INVALID_ARG, "sr_mser_last_regions: bad arguments");
    *count = (int64_t)ctx->mser_last.size();
    const size_t m = std::min<size_t>(ctx->mser_last.size(), (size_t)cap);
    if (m) std::copy(ctx->mser_last.begin(), ctx->mser_last.begin() + m, h_regions);
    return SR_OK;
}

int sr_mser_workspace(sr_ctx *ctx, void **d_ptr, size_t *bytes)
{
    CTX_ENTER(ctx);
    if (!d_ptr || !bytes) return sr_set_error(SR_ERR_INVALID_ARG, "sr_mser_workspace: null output");
    *d_ptr = ctx->mser_ws.d;
    *bytes = ctx->mser_ws.cap;
    return SR_OK;
}

int sr_mser_tree_u8(sr_ctx *ctx, const uint8_t *d_img, int64_t stride, int h, int w, int cn, int polarity, sr_mser_node *h_nodes,
                    int64_t cap, int64_t *count)
{
    CTX_ENTER(ctx);
    if (bad_image(d_img, stride, h, w, cn) || !count || cap < 0 || (cap > 0 && !h_nodes) || polarity < 0 || polarity > 1)
        return sr_set_error(SR_ERR_INVALID_ARG, "sr_mser_tree_u8: bad arguments");
    sr_mser_params dp;
    sr_mser_default_params(&dp);
    SRCHK(mser_check("sr_mser_tree_u8", h, w, &dp));
    MserPlan pl;
    mser_layout(h, w, &pl);
    MsView v;
    SRCHK(build_tree(ctx, "sr_mser_tree_u8", d_img, stride, h, w, cn, polarity, pl, &v));
    unsigned nn = 0;
    HIPCHK(hipMemcpyAsync(&nn, v.ctr + MS_CTR_NODES, sizeof(nn), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(stream_sync(ctx));
    if (nn > (unsigned)v.node_cap) return sr_set_error(SR_ERR_HIP, "sr_mser_tree_u8: node table overflow (%u nodes)", nn);
    *count = (int64_t)nn;
    if ((int64_t)nn > cap) return SR_OK;
    std::vector<MserNode> nodes(nn);
    if (nn) {
        HIPCHK(hipMemcpyAsync(nodes.data(), v.nodes, (size_t)nn * sizeof(MserNode), hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(stream_sync(ctx));
    }
    for (const MserNode &n : nodes)
        if (n.parent < -1 || n.parent >= (int)nn) return sr_set_error(SR_ERR_HIP, "sr_mser_tree_u8: a node's parent is outside the table");
    mser_canonical_tree(nodes, h_nodes);
    return SR_OK;
}
