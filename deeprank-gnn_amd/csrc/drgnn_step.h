// The phase routines the aggregation-first fused step kernels share (drgnn_step2.h: sGAT / FoutNet, drgnn_step3.h: GINet):
// the launch description (StepArgs), the dense product, the gathers, the depth-1 pool + readout, the readout exchange between
// the branch workgroups of a graph and the pieces of the FC head, plus the host-side bounds the launch plan is made from
// (drgnn_capi.hip, step_pick).  Same math as net_forward_graph + head_graph + net_backward_graph (drgnn_net.h; reference
// ginet.py:103-139, sGAT.py:119-137, foutnet.py:108-124 and their autograd), with every intermediate kept in LDS.
// dW_fc1 = dhid^T readout is left to the update kernel (it only needs dhid [B,H] and the readout [B,R]), so the head writes a
// compact slab  [dhid H][dW2 O*H][db2 O][loss][weight]  (head_compact_floats).
// The routines are device code only: the host emulation (DRGNN_EMU) steps a fused launch through the launch pair's
// per-graph routines instead (train_step_impl).
#ifndef DRGNN_STEP_H
#define DRGNN_STEP_H

#include "drgnn_net.h"

// ablation profiling (tools/ablate_step.sh): -DDRGNN_SKIP=k compiles the step kernel WITHOUT the work
// of phase k (barriers stay); the drop in kernel time is what that phase costs.  Never set in the product.
#ifndef DRGNN_SKIP
#define DRGNN_SKIP (-1)
#endif
#define PH(k) if (DRGNN_SKIP != (k))
// -DDRGNN_EXIT_AFTER=k: every workgroup returns after barrier k (cumulative timeline of the phases)
#ifndef DRGNN_EXIT_AFTER
#define DRGNN_EXIT_AFTER (-1)
#endif
// (the checksum over the whole scratch keeps every earlier LDS store alive in the truncated kernel)
#define EXIT_AFTER(k)                                                                          \
    do {                                                                                       \
        if (DRGNN_EXIT_AFTER == (k)) {                                                         \
            float acc_ = 0.0f;                                                                 \
            if ((k) > 0) { FOR_TID(i_, (int)(s.end - scratch)) { acc_ += scratch[i_]; } }      \
            if (acc_ == 12345.678f) a.hf.pred[0] = acc_;                                       \
            return;                                                                            \
        }                                                                                      \
    } while (0)

struct StepArgs {
    drgnn_net_desc net;
    const float* x;              // [Ntot, F]
    TopoView tv;
    int64_t n_nodes;
    int n_graphs;
    float* partials;             // [B*n_branch][P] conv weight-gradient slabs (net_partial_floats)
    int n_partial;
    HeadFused hf;                // hf.readout: [B][R] OUTPUT; hf.partials: [B][head_compact_floats]
    unsigned long long* xchg;    // [B][n_branch][H] tagged fc1 half-products (zero-initialised once by the owner)
    int xchg_stride;             // node-split layout (drgnn_step2.h): exchange words per graph (step2_xchg_words)
    int32_t* step2;              // [0] steps completed so far (read)   [1] index of this step (written)   [2] sticky fault bits
    // cached-topology mode: slot g of the launch is graph gather_ids[g] of the workspace `tv` describes (a whole
    // resident set, ws_graphs graphs); null: slot g = graph g of a per-mini-batch workspace
    const int32_t* gather_ids;
    int ws_graphs;
    // aggregation tiles of the workspace (DRGNN_TOPO_TILES): S [tile_nodes][F] | D [tile_nodes] | C [tile_nodes], node order
    const float* tiles;
    int64_t tile_nodes;
};

HD int64_t head_compact_floats(int R, int H, int O) { (void)R; return (int64_t)H + (int64_t)O * H + O + 2; }

#define STEP_XPLD (DRGNN_H1 + 4)     // pooled features: 20-float rows (conflict-free 128-bit row reads)
// the fc1 column block [H][STEP_WBLD] and, after the head, the partial tiles of the K-split products (256 floats per
// (tile, K slice) unit) share one area: at least 8 units, all 16 when H makes it that large anyway
#define STEP_WBLD (DRGNN_H2 + 4)     // row stride of the fc1.weight column block in LDS (16-byte aligned rows)
HD int step_gp_words(int H) { return H * STEP_WBLD > 2048 ? H * STEP_WBLD : 2048; }
HD int step_pad4(int n) { return (n + 3) & ~3; }
HD int step_pad16(int n) { return (n + 15) & ~15; }

template <bool NARROW> struct StepIdx { typedef int type; };
template <> struct StepIdx<true> { typedef unsigned short type; };

// LDS words of one workgroup of the product-first step kernel of rounds 2 - 3 (no longer built): what the exported
// drgnn_net_step_lds_bytes reports, and the capacity bound of the host emulation's fused step (drgnn_capi.hip, step_pick).
#define STEP_CARVE_LIST(X)                                                                     \
    X(misc, 128, 1)                                                                            \
    X(xr, R, 1)                                                                                \
    X(hid, H, 1)                                                                               \
    X(dhid, H, 1)                                                                              \
    X(hb1, H, 1)                                                                               \
    X(bsum, DRGNN_NWAVES * DRGNN_H2, !gin)                                                     \
    X(wb, step_gp_words((int)H), 1)                                                            \
    X(w1t, DRGNN_H1 * xld, 1)                                                                  \
    X(ws1t, DRGNN_H1 * xld, !gin)                                                              \
    X(b1, DRGNN_H1, !gin)                                                                      \
    X(w2t, DRGNN_H2 * STEP_XPLD, gin)                                                          \
    X(w2n, DRGNN_H1 * (DRGNN_H2 + 4), gin)                                                     \
    X(wc2t, DRGNN_H2 * (DRGNN_H2 + 4), !gin)                                                   \
    X(wc2n, DRGNN_H2 * (DRGNN_H2 + 4), !gin)                                                   \
    X(b2, DRGNN_H2, !gin)                                                                      \
    X(xs, (long)(capN + 4) * xld, 1)                                                           \
    X(rp0, capN + 1, 1)                                                                        \
    X(cx0, (sg ? (capE + 1) / 2 : capE), 1)                                                    \
    X(ew0, capE, sg)                                                                           \
    X(cp0, capN + 1, 1)                                                                        \
    X(rx0, (sg ? (capE + 1) / 2 : capE), 1)                                                    \
    X(ts0, (sg ? (capE + 1) / 2 : capE), sg)                                                   \
    X(ct0, capE, !gin)                                                                         \
    X(mp0, capC + 1, 1)                                                                        \
    X(mem0, capN, 1)                                                                           \
    X(rp1, capC + 1, 1)                                                                        \
    X(cx1, (sg ? (capE + 1) / 2 : capE), 1)                                                    \
    X(ew1, capE, sg)                                                                           \
    X(cp1, capC + 1, 1)                                                                        \
    X(rx1, (sg ? (capE + 1) / 2 : capE), 1)                                                    \
    X(ts1, (sg ? (capE + 1) / 2 : capE), sg)                                                   \
    X(mp1, capC + 1, 1)                                                                        \
    X(mem1, capC, 1)                                                                           \
    X(a0, ((long)capC * DRGNN_H1 + 1) / 2, 1)                                                    \
    X(a1, ((long)capC * DRGNN_H2 + 1) / 2, 1)                                                    \
    X(u1, (long)(capN + 4) * hc1, 1)                                                           \
    X(z1, (long)capN * DRGNN_H1, 1)                                                            \
    X(dv0, capN, !gin)                                                                         \
    X(sc0, capN, !gin)                                                                         \
    X(xp, (long)(capC + 4) * STEP_XPLD, 1)                                                     \
    X(u2, (long)(capC + 4) * (DRGNN_H2 + 4), 1)                                                \
    X(z2, (long)(capC + 4) * (DRGNN_H2 + 4), 1)                                                \
    X(p2, (gin ? ((long)capC * DRGNN_H2 > (long)(capC + 4) * STEP_XPLD ? (long)capC * DRGNN_H2 : (long)(capC + 4) * STEP_XPLD) \
               : (long)(capC + 4) * (DRGNN_H2 + 4)), 1)                                        \
    X(dv1, capC, !gin)                                                                         \
    X(sc1, capC, !gin)                                                                         \
    X(hw2, (long)O * H, 1)                                                                     \
    X(hb2, O, 1)

HD int64_t step_scratch_words(int kind, int64_t F, int64_t capN, int64_t capE, int64_t capC, int64_t R,
                              int64_t H, int64_t O) {
    const int64_t hc1 = (kind == DRGNN_GINET) ? DRGNN_H1 : 2 * DRGNN_H1;
    const int64_t hc2 = (kind == DRGNN_GINET) ? DRGNN_H2 : 2 * DRGNN_H2;
    const int sg = (kind == DRGNN_SGAT) ? 1 : 0;
    const int gin = (kind == DRGNN_GINET) ? 1 : 0;
    const int64_t xld = step_pad16((int)F) + 4;
    int64_t w = 0;
#define X(name, words, cond) w += (cond) ? (((int64_t)(words) + 3) & ~(int64_t)3) : 0;   /* 16-byte aligned arrays */
    STEP_CARVE_LIST(X)
#undef X
    return w + 16;
}

// per-graph scalars of the loss, fetched during staging:  misc = [bad (int)][y or class id][wy][denom]
#define STEP_M_BAD 0
#define STEP_M_Y 1
#define STEP_M_WY 2
#define STEP_M_DENOM 3
#define STEP_WB_J 4        // float4 per lane: H * 8 <= STEP_WB_J * 1024  (H <= 512)

// host side of the same conditions (net_burst_ok + the head's), from the batch-wide bounds
static inline bool step_burst_guaranteed(int kind, const float* x, int F, int capN, int capE, int capC, int H, int O) {
    if (H != ((kind == DRGNN_GINET) ? 128 : 64)) return false;      // the specialised kernels carry the reference head width only
    return ((((uintptr_t)x) & 15) == 0) && (F % 4 == 0) && (F * DRGNN_H1 <= DRGNN_BCAP) && ((long)capN * F <= 16L * DRGNN_BCAP) &&
           (capN + 1 <= DRGNN_BCAP) && (capE <= 2 * DRGNN_BCAP) && (capC * DRGNN_H1 <= 4 * DRGNN_BCAP) &&
           O * H <= 2 * DRGNN_BCAP && H * 8 <= STEP_WB_J * DRGNN_BCAP;
}

// Capacity class of the LDS layout (the CLS argument of the kernels).  0: laid out for the run-time capacities (capN, capE,
// capC = the maxima of the batch, exact fit: that is what lets 200-node graphs into 160 KB at all).  1: the fixed layout
// STEP_CLS_N / _E / _C -- the largest graph shape the kernels fit at feature widths up to 48 -- with every array offset an
// immediate instead of ~40 pinned registers and run-time address arithmetic: 0.2 - 0.4 us per step.  The host
// takes it whenever the batch's maxima lie inside the class (step_pick); LDS is one workgroup per CU either way.
#define STEP_CLS_N 200
#define STEP_CLS_E 1024
#define STEP_CLS_C 52

#ifndef DRGNN_EMU
#define STEP_PIN(x) asm volatile("" : "+v"(x))

// ---- dense products of the step kernel ----------------------------------------------------------
// Layout rules that let the MFMA loops run without lane predicates: row-major operands have 16-byte aligned rows (stride
// % 4 == 0) and their K extent is zero padded to a multiple of 16 -- a lane fetches 4 consecutive k with ONE 128-bit LDS
// read and feeds them to 4 MFMA steps (the k order inside a 16-chunk is permuted the same way for A and B, which does not
// change the sum's terms).  Rows past M of a last tile are computed from whatever LDS holds and their stores discarded.

// C[M x 16*NT] (row stride ldc) = A[M x K] * Bt^T,  A rows of stride lda, Bt[n][k] rows of stride ldbt
// RELU: C = relu(...) with NaN passing through, like torch
// wave_shift: tile unit u goes to wave (u + wave_shift) mod 16 -- callers that issue two products in one phase start the
// second one where the first one's units end, so that all 16 waves get tiles
template <bool RELU = false>
DEV void step_gemm_nn(int M, int NT, int K, const float* A, int lda, const float* Bt, int ldbt, float* C, int ldc,
                      int* dummy, const float* bias = nullptr, const float* nan_rows = nullptr, int wave_shift = 0) {
    // nan_rows: rows i with nan_rows[i] == 0 are written as NaN (FoutLayer's mean over an empty neighbourhood)
    const int wave = (__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) - wave_shift) & (DRGNN_NWAVES - 1);
    const int lane = threadIdx.x & 63;
    const int lr = lane & 15, lq = lane >> 4;
    const int units = ((M + 15) >> 4) * NT;
    for (int u = wave; u < units; u += DRGNN_NWAVES) {
        const int ti = (NT == 1) ? u : (u >> 1), tj = (NT == 1) ? 0 : (u & 1);      // NT is 1 or 2
        const float* ap = A + (ti * 16 + lr) * lda + 4 * lq;
        const float* bp = Bt + (tj * 16 + lr) * ldbt + 4 * lq;
        drgnn_f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        for (int k0 = 0; k0 < K; k0 += 32) {
            const drgnn_f4 a0 = *(const drgnn_f4*)(ap + k0), b0 = *(const drgnn_f4*)(bp + k0);
            const bool two = k0 + 16 < K;
            drgnn_f4 a1 = a0, b1 = b0;
            if (two) { a1 = *(const drgnn_f4*)(ap + k0 + 16); b1 = *(const drgnn_f4*)(bp + k0 + 16); }
#pragma unroll
            for (int j = 0; j < 4; ++j) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[j], b0[j], acc, 0, 0, 0);
            if (two) {
#pragma unroll
                for (int j = 0; j < 4; ++j) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a1[j], b1[j], acc, 0, 0, 0);
            }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int ci = ti * 16 + lq * 4 + r;
            float* p = (ci < M) ? C + ci * ldc + tj * 16 + lr : (float*)dummy + lane;
            float v = acc[r];
            if (bias) v += bias[tj * 16 + lr];
            if (nan_rows && ci < M && nan_rows[ci] == 0.0f) v = DRGNN_NAN;
            if (RELU) v = (v < 0.0f) ? 0.0f : v;
            *p = v;
        }
    }
}

// ---- GINet's second convolution, aggregation first ------------------------------------------------
// relu(A (XP W2)) = relu((A XP) W2): summing the 16-wide pooled rows BEFORE the dense product halves the
// bytes the LDS gathers move (64 instead of 128 per edge), forward and backward alike.
// dst[i][0:16] = sum over CSR row i of src[col][0:16]; rows of LD floats, 4 lanes per row
template <int LD, class IdxT>
DEV void step_gather_rows(int n, const int* rp, const IdxT* col, const float* src, float* dst) {
    // 16 lanes per pooled node: 4 channel groups x 4 interleaved slices of the
    // row's entry list (few, long rows), slice sums combined in fixed order by two DPP steps
    const int items = ((n * 16) + 63) & ~63;
    for (int item = threadIdx.x; item < items; item += DRGNN_NTHREADS) {
        const int i = item >> 4, sl = (item >> 2) & 3, c = (item & 3) * 4;
        float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
        if (i < n) {
            const int lo = rp[i], hi = rp[i + 1];
            for (int k = lo + sl; k < hi; k += 4) {
                const drgnn_f4 v = *(const drgnn_f4*)(src + ROW24(col[k], LD) + c);
                a0 += v[0]; a1 += v[1]; a2 += v[2]; a3 += v[3];
            }
        }
        a0 += dpp_take<0x128>(a0); a1 += dpp_take<0x128>(a1); a2 += dpp_take<0x128>(a2); a3 += dpp_take<0x128>(a3);
        a0 += dpp_take<0x124>(a0); a1 += dpp_take<0x124>(a1); a2 += dpp_take<0x124>(a2); a3 += dpp_take<0x124>(a3);
        if (sl == 0 && i < n) *(drgnn_f4*)(dst + i * LD + c) = drgnn_f4{a0, a1, a2, a3};
    }
}

// Depth-1 max-pool with argmax (first maximum in ascending member order, NaN never wins, empty cluster -> 0,
// arg = -1 where no gradient can flow) fused with the graph readout = mean over the depth-1 clusters.
// SKIP0: rows of nodes without out-edges (rp[m+1] == rp[m]) count as NaN, i.e. never win (FoutNet)
// pub: (GINet) this branch's DRGNN_H2 exchange words -- every readout value is published to the partner branch's workgroup
// the moment it exists (tag = index of this step), so that it travels while both workgroups pass the phase's barrier
DEV void xchg_publish(unsigned long long* slot, uint32_t tag, float v);
// a1ld: layout of the argmax array.  0: arg[k][32] (cluster-major: every kernel family but one); > 0: arg[c][a1ld] (column-major,
// a1ld >= C1: drgnn_step3.h -- its readers walk the clusters of ONE column with consecutive lanes, which in the cluster-major
// layout lands 16 lanes on two LDS banks, profiles/r05_lds_conflicts.txt)
template <int LDZ, bool SKIP0 = false>
DEV void step_pool_readout(int C1, const int* mp, const int* mem, const float* z, short* arg, const float* misc,
                           float* xr, float* g_readout, const int* rp = nullptr, unsigned long long* pub = nullptr,
                           uint32_t tag = 0u, int a1ld = 0) {
    int bad; memcpy(&bad, &misc[STEP_M_BAD], 4);
    const float inv = 1.0f / (float)(C1 > 0 ? C1 : 1);
    for (int t = threadIdx.x; t < DRGNN_H2 * 16; t += DRGNN_NTHREADS) {      // 512 lanes: whole waves
        const int c = t >> 4, kk = t & 15;
        float acc = 0.0f;
        for (int k = kk; k < C1; k += 16) {
            float best = DRGNN_NEG_INF;
            int am = -1;
            // members in batches of four independent (member -> value) chains; a short last batch repeats the cluster's last
            // member, which cannot win again (strict >): same maximum, same first-maximum argmax -- without the 1 - 3 serial
            // LDS round trips of a remainder loop (SYN's depth-1 clusters have 3 members: all remainder)
            const int plo = mp[k], phi = mp[k + 1];
            for (int p = plo; p < phi; p += 4) {
                int mm[4];
                float vv[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) mm[j] = mem[(p + j < phi) ? p + j : phi - 1];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    vv[j] = z[ROW24(mm[j], LDZ) + c];
                    if (SKIP0 && rp[mm[j] + 1] == rp[mm[j]]) vv[j] = DRGNN_NAN;      // (NaN never wins)
                }
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (vv[j] > best) { best = vv[j]; am = mm[j]; }
            }
            if (am < 0) best = 0.0f;
            arg[a1ld ? c * a1ld + k : k * DRGNN_H2 + c] = (short)((best > 0.0f) ? am : -1);
            acc += best;
        }
        acc = lanes16_sum(acc) * inv;
        if (bad) acc = DRGNN_NAN;
        if (kk == 0) {
            if (pub) xchg_publish(pub + c, tag, acc);      // first: the store that has the farthest to go
            xr[c] = acc; out_store(&g_readout[c], acc);
        }
    }
}

// ---- readout exchange between the branch workgroups of a graph -----------------------------------
DEV void xchg_publish(unsigned long long* slot, uint32_t tag, float v) {
    const unsigned long long w = ((unsigned long long)tag << 32) | (unsigned long long)__float_as_uint(v);
    __hip_atomic_store(slot, w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// Spins until the partner has published its value of THIS step.  The branch workgroups of a graph are 8 block ids apart
// (same XCD); up to 64 graphs the launch fits the device in one wave and the partner is resident.  Larger batches rely
// on the dispatcher handing out blocks in id order (it does; HIP does not promise it): the partner then becomes resident
// as soon as any earlier workgroup retires, long before this wait's bound (~0.3 s of the 100 MHz wall clock).  On expiry
// the value is NaN (a NaN loss instead of a hung queue) AND bit DRGNN_FAULT_EXCHANGE is raised in the sticky fault word
// step2[2], which the trainers check once per epoch.
DEV float xchg_wait(unsigned long long* slot, uint32_t tag, int32_t* fault) {
    const unsigned long long t0 = wall_clock64();
    for (;;) {
        const unsigned long long w = __hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if ((uint32_t)(w >> 32) == tag) return __uint_as_float((uint32_t)w);
        if (wall_clock64() - t0 > 30000000ull) { atomicOr(fault, DRGNN_FAULT_EXCHANGE); return DRGNN_NAN; }
        __builtin_amdgcn_s_sleep(1);
    }
}
// the same in two halves: the first poll is REQUESTED early (its L2 round trip overlaps the caller's own work) ...
DEV unsigned long long xchg_peek(const unsigned long long* slot) {
    return __hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// ... and completed here: spins only if that first answer was not this step's word yet
DEV float xchg_finish(unsigned long long* slot, unsigned long long w, uint32_t tag, int32_t* fault) {
    if ((uint32_t)(w >> 32) == tag) return __uint_as_float((uint32_t)w);
    return xchg_wait(slot, tag, fault);
}

// ---- head pieces -----------------------------------------------------------------------------
// Column block of fc1.weight owned by this branch: wb[h][c] = W1[h][br*32 + c]  (LDS, rows of
// STEP_WBLD floats).  Loaded as float4 (8 lanes cover the 128 contiguous bytes of a row).
// WJ: float4 per lane; 1 covers H <= 128 (the reference heads -- what the width-specialised kernels are launched
// for), STEP_WB_J the general case.  Twelve VGPRs apart, which is what the sGAT / FoutNet kernels spill otherwise.
template <int WJ> struct WBlockRegs { drgnn_f4 v[WJ * DRGNN_BSCALE]; };
template <int WJ> DEV void step_wblock_load(WBlockRegs<WJ>& wr, const HeadFused& hf, int br) {
    const bool vec = ((((uintptr_t)hf.w1) & 15) == 0);       // R = 32*n_branch floats: rows stay 16-byte aligned
#pragma unroll
    for (int j = 0; j < WJ * DRGNN_BSCALE; ++j) {
        const int t = threadIdx.x + j * DRGNN_NTHREADS;
        const int h = t >> 3, q = t & 7;
        drgnn_f4 v = {0.f, 0.f, 0.f, 0.f};
        if (h < hf.H) {
            const float* src = hf.w1 + (long)h * hf.R + br * DRGNN_H2 + 4 * q;
            if (vec) v = *(const drgnn_f4*)src;
            else { v[0] = src[0]; v[1] = src[1]; v[2] = src[2]; v[3] = src[3]; }
        }
        wr.v[j] = v;
    }
}
template <int WJ> DEV void step_wblock_store(const WBlockRegs<WJ>& wr, const HeadFused& hf, int br, float* wb) {
    (void)br;
#pragma unroll
    for (int j = 0; j < WJ * DRGNN_BSCALE; ++j) {
        const int t = threadIdx.x + j * DRGNN_NTHREADS;
        const int h = t >> 3, q = t & 7;
        if (h < hf.H) *(drgnn_f4*)(wb + h * STEP_WBLD + 4 * q) = wr.v[j];
    }
}

// hid = dropout(relu(b1 + P0 + P1)),  P_br = W1[:, br*32:(br+1)*32] readout_br.  8 lanes per hidden unit, DPP sum inside the
// lane group.  GINet: BOTH branch workgroups of a graph evaluate the whole of fc1 -- the own half from the column block in
// LDS (`wb`, which the head's backward needs anyway) and the own readout, the partner's half from the partner's column
// block held in REGISTERS since the second burst (`wo`) and the partner's readout, which the partner published value by
// value at the end of its pooling phase (step_pool_readout) -- one hand-off of 32 values that is already in flight while
// this workgroup passes the barrier and forms its own half, instead of 128 half products exchanged afterwards.
// `xg`: the [n_branch][DRGNN_H2] exchange words of graph g.  Lanes 0..31 of EVERY wave poll the partner's 32 words (a wave
// cannot learn them from another wave without a barrier) and hand them to the lane groups with four lane reads.
// HC: the head's width as a compile-time constant (0: taken from the descriptor).
template <int HC, int WJ>
DEV void step_head_fc1_t(const HeadFused& hf, int g, int br, int nb, const float* wb, const WBlockRegs<WJ>& wo,
                         const float* b1, const float* xr, float* hid, unsigned long long* xg, uint32_t tag, uint32_t step,
                         uint32_t thresh, float keep_scale, int32_t* fault) {
    const int H = HC ? HC : hf.H;
    const int lane = threadIdx.x & 63;
    unsigned long long* const slot = xg + (long)(1 - br) * DRGNN_H2 + (lane & (DRGNN_H2 - 1));
    unsigned long long w0 = 0ull;
    if (nb > 1 && lane < DRGNN_H2) w0 = xchg_peek(slot);        // in flight behind the own half below
    const int items = (H * 8 + 63) & ~63;         // whole waves: the lane-group sums need every lane
    drgnn_f4 xo = {0.f, 0.f, 0.f, 0.f};
    bool have_other = false;
    int j = 0;
    for (int t = threadIdx.x; t < items; t += DRGNN_NTHREADS, ++j) {
        const int h = t >> 3, q = t & 7;
        float acc = 0.0f;
        if (h < H) {
            const drgnn_f4 w = *(const drgnn_f4*)(wb + h * STEP_WBLD + 4 * q);
            const drgnn_f4 x = *(const drgnn_f4*)(xr + 4 * q);
            acc = fmaf(w[0], x[0], fmaf(w[1], x[1], fmaf(w[2], x[2], w[3] * x[3])));
        }
        acc = lanes8_sum(acc);
        float v = acc;
        if (nb > 1) {
            if (!have_other) {       // (wave-uniform) the partner's readout: lanes 0..31 poll, every lane takes its float4
                float pv = 0.0f;
                PH(7) { if (lane < DRGNN_H2) pv = xchg_finish(slot, w0, tag, fault); }
                const int src = (lane & 7) * 4;
                xo[0] = __shfl(pv, src, 64); xo[1] = __shfl(pv, src + 1, 64);
                xo[2] = __shfl(pv, src + 2, 64); xo[3] = __shfl(pv, src + 3, 64);
                have_other = true;
            }
            float other = 0.0f;
            if (h < H) {
                const drgnn_f4 w = wo.v[j < WJ * DRGNN_BSCALE ? j : 0];
                other = fmaf(w[0], xo[0], fmaf(w[1], xo[1], fmaf(w[2], xo[2], w[3] * xo[3])));
            }
            other = lanes8_sum(other);
            v = (br == 0) ? acc + other : other + acc;       // P0 + P1 in both workgroups
        }
        if (q == 0 && h < H) {
            v += b1[h];
            v = v > 0.0f ? v : 0.0f;
            if (thresh) v = drgnn_keep(hf, step, g, H, h, thresh) ? v * keep_scale : 0.0f;
            hid[h] = v;
        }
    }
}
// WREF: the fc1 width of the reference net of this kind (128 for GINet, 64 for sGAT / FoutNet) -- the one width a
// kernel carries a specialised copy for besides the generic routines (every copy is instruction-cache footprint)
// ONLY: the host has checked H == WREF for this launch (width-specialised kernels): no generic copy at all
template <int WREF, bool ONLY, int WJ>
DEV void step_head_fc1(const HeadFused& hf, int g, int br, int nb, const float* wb, const WBlockRegs<WJ>& wo, const float* b1,
                       const float* xr, float* hid, unsigned long long* xg, uint32_t tag, uint32_t step,
                       uint32_t thresh, float keep_scale, int32_t* fault) {
    if (ONLY || hf.H == WREF) step_head_fc1_t<WREF, WJ>(hf, g, br, nb, wb, wo, b1, xr, hid, xg, tag, step, thresh, keep_scale, fault);
    else step_head_fc1_t<0, WJ>(hf, g, br, nb, wb, wo, b1, xr, hid, xg, tag, step, thresh, keep_scale, fault);
}

// outs = W2 hid + b2, loss, d loss / d outs, then dhid = relu'/dropout' (W2^T douts).  Device: every
// wave evaluates outs redundantly (lane o keeps outs[o] / douts[o]) so that no barrier separates
// them from their consumers.  Branch 0 writes predictions and the head slab.
template <int HC, int OC>
DEV void step_head_loss_t(const HeadFused& hf, int g, int br, const float* hid, const float* w2, const float* b2,
                          const float* misc, float keep_scale, float* dhid, float* p_dhid, float* p_hw2,
                          float* p_hb2, float* p_loss) {
    const int H = HC ? HC : hf.H, O = OC ? OC : hf.O;
    if (__builtin_expect(!hf.train, 0)) {            // inference: predictions only
        if (br == 0) {
            FOR_TID(o, O) {
                float acc = b2[o];
                for (int h = 0; h < H; ++h) acc = fmaf(hid[h], w2[o * H + h], acc);
                if (hf.sigmoid && hf.task != DRGNN_TASK_CLASS) acc = drgnn_sigmoid(acc);
                out_store(&hf.pred[(long)g * O + o], acc);
            }
        }
        return;
    }
    // (DRGNN_TASK_GRAD: d loss / d pred comes from the caller's autograd -- misc[STEP_M_Y] holds it when O == 1, the row
    // hf.y_reg[g * O ..] otherwise -- and the loss slot is written as 0; regression in every other respect)
    const bool ext = hf.task == DRGNN_TASK_GRAD;
    const bool sig = hf.sigmoid && hf.task != DRGNN_TASK_CLASS;
    const float denom = misc[STEP_M_DENOM], wy = misc[STEP_M_WY];
    // only the waves that own a hidden unit below (wave 0 also writes the predictions) need the outputs: the
    // others would just repeat the same ~150 instructions on the same SIMDs
    if ((int)(threadIdx.x & ~63u) >= H && threadIdx.x >= 64) return;
    const int lane = threadIdx.x & 63;
    if (HC != 0 && HC <= 128 && OC == 1 && hf.task != DRGNN_TASK_CLASS) {
        // The reference heads (one output, MSE): this phase is ONE dependent chain in one or two waves while fourteen wait,
        // so every LDS operand is requested up front (one round trip instead of six), the wave sum runs once (the loss of a
        // single output needs none) and no value travels through a lane read: out and d loss / d out are wave-uniform.
        // Same operations in the same order as the general path below: bit-identical results.
        constexpr int NH = (HC > 0) ? (HC + 63) / 64 : 1;      // (HC == 0 never takes this path)
        float hv[NH], wv[NH];
#pragma unroll
        for (int j = 0; j < NH; ++j) { hv[j] = hid[lane + 64 * j]; wv[j] = w2[lane + 64 * j]; }
        const float bias = b2[0], yv = misc[STEP_M_Y];
        float acc = 0.0f;
#pragma unroll
        for (int j = 0; j < NH; ++j) acc = fmaf(hv[j], wv[j], acc);
        float out = lanes64_sum(acc) + bias;
        if (sig) out = drgnn_sigmoid(out);
        const float inv = 1.0f / (float)(hf.B * O);
        const float d = out - yv;
        const float dout = (ext ? yv : 2.0f * d * inv) * (sig ? out * (1.0f - out) : 1.0f);
        const int wv_id = (int)(threadIdx.x >> 6);
        float hme = hv[0], wme = wv[0];
#pragma unroll
        for (int j = 1; j < NH; ++j) { if (wv_id == j) { hme = hv[j]; wme = wv[j]; } }
        const int h = (int)threadIdx.x;                       // < HC: the waves past H have returned
        const float dh = (hme != 0.0f) ? fmaf(dout, wme, 0.0f) * keep_scale : 0.0f;     // relu' and dropout mask
        dhid[h] = dh;
        if (br == 0) {
            out_store(&p_hw2[h], dout * hme);
            out_store(&p_dhid[h], dh);
            if (threadIdx.x == 0) {
                out_store(&hf.pred[(long)g], out);
                out_store(&p_hb2[0], dout);
                out_store(&p_loss[0], ext ? 0.0f : (d * d * inv));
                out_store(&p_loss[1], 1.0f);
            }
        }
        return;
    }
    float my_out = 0.0f;
    for (int o = 0; o < O; ++o) {
        float acc = 0.0f;
        for (int h = lane; h < H; h += 64) acc = fmaf(hid[h], w2[o * H + h], acc);
        acc = lanes64_sum(acc) + b2[o];
        if (lane == o) my_out = acc;
    }
    if (sig) my_out = drgnn_sigmoid(my_out);
    float my_dout = 0.0f, loss, wsum = 1.0f;
    if (ext) {
        loss = 0.0f;
        my_dout = lane < O ? hf.y_reg[(long)g * O + lane] * (sig ? my_out * (1.0f - my_out) : 1.0f) : 0.0f;
    } else if (__builtin_expect(hf.task == DRGNN_TASK_REG, 1)) {      // (layout hint: the exp / log code of the other branch goes out of line)
        const float inv = 1.0f / (float)(hf.B * O);
        const float d = my_out - misc[STEP_M_Y];
        loss = lanes64_sum(lane < O ? d * d * inv : 0.0f);
        my_dout = lane < O ? 2.0f * d * inv * (sig ? my_out * (1.0f - my_out) : 1.0f) : 0.0f;
    } else {
        const int yc = __builtin_amdgcn_readfirstlane(__float_as_int(misc[STEP_M_Y]));
        const float mx = lanes64_max(lane < O ? my_out : DRGNN_NEG_INF);
        const float se = lanes64_sum(lane < O ? expf(my_out - mx) : 0.0f);
        const float lse = logf(se) + mx;
        loss = wy * (lse - lane_get(my_out, yc)) / denom;
        my_dout = lane < O ? wy * (expf(my_out - lse) - (lane == yc ? 1.0f : 0.0f)) / denom : 0.0f;
        wsum = wy;
    }
    if (br == 0 && (int)threadIdx.x < O) {
        out_store(&hf.pred[(long)g * O + threadIdx.x], my_out);
        out_store(&p_hb2[threadIdx.x], my_dout);
    }
    if (br == 0 && threadIdx.x == 0) { out_store(&p_loss[0], loss); out_store(&p_loss[1], wsum); }
    for (int h0 = 0; h0 < H; h0 += DRGNN_NTHREADS) {      // uniform trip count: lane_get below is wave-wide
        const int h = h0 + (int)threadIdx.x;
        const bool ok = h < H;
        const float hv = ok ? hid[h] : 0.0f;
        float acc = 0.0f;
        for (int o = 0; o < O; ++o) {
            const float dout = lane_get(my_dout, o);
            if (ok) {
                acc = fmaf(dout, w2[o * H + h], acc);
                if (br == 0) out_store(&p_hw2[(long)o * H + h], dout * hv);
            }
        }
        if (ok) {
            const float dh = (hv != 0.0f) ? acc * keep_scale : 0.0f;     // relu' and dropout mask
            dhid[h] = dh;
            if (br == 0) out_store(&p_dhid[h], dh);
        }
    }
}
template <int WREF, bool ONLY>
DEV void step_head_loss(const HeadFused& hf, int g, int br, const float* hid, const float* w2, const float* b2,
                        const float* misc, float keep_scale, float* dhid, float* p_dhid, float* p_hw2,
                        float* p_hb2, float* p_loss) {
    if (__builtin_expect(hf.H == WREF && hf.O == 1, 1))
        step_head_loss_t<WREF, 1>(hf, g, br, hid, w2, b2, misc, keep_scale, dhid, p_dhid, p_hw2, p_hb2, p_loss);
    else
        step_head_loss_t<0, 0>(hf, g, br, hid, w2, b2, misc, keep_scale, dhid, p_dhid, p_hw2, p_hb2, p_loss);
}
#endif  // !DRGNN_EMU

#endif
