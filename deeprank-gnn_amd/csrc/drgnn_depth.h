// drgnn_depth.h -- residue depth: the reference's `depth` node feature (Biopython's residue depth: the mean, over the
// atoms of a residue, of the distance to the molecular surface MSMS computes) for chosen residues of a ragged batch of
// complexes, from a dot surface of the solvent-accessible surface restricted to its outer component.
// tests/depth_ref.py states the rule in numpy float64.
//
//   radii     rad f64 [n_radii], atom t reads entry t % n_radii; 0: the atom takes no part in the surface (its depth
//             is still measured).  R_i = r_i + probe
//   dots      p_ik = x_i + R_i S_k over the unit-dot table S f64 [n_dots, 3] the caller hands in; dot (i, k) is
//             accessible when |p_ik - x_j|^2 >= R_j^2 for every other participating atom j of the complex
//   links     two accessible dots are linked when |p - q|^2 <= link^2; a component is labelled by its smallest dot id
//   outer     the component with the most dots, ties to the smallest label (all = 1: every accessible dot is kept)
//   depth     of an atom: sqrt(min over the kept dots of |x - p|^2) - probe (+inf without a dot); of a residue: the mean
//             over its atoms, summed in order
// Every product and sum is one fp64 operation on the fp32 coordinates, d^2 = (dx dx + dy dy) + dz dz, no contraction into
// fused multiply-adds: the accessible set, the links and the labels are the integers the rule gives, and the depth has the
// rule's bits.  The atom scans are pre-filters with a margin of 1e-3 of the distance they test, far above the rounding.
//
// Three launches per call:
//   k_depth_dots        one wave per atom (16 atoms per workgroup).  For every word of 64 dots the wave scans the atoms of
//                       the complex 64 at a time (a lane tests one atom: can its sphere reach mine?), then every lane
//                       tests its dot against the atoms of the ballot; the word of the mask is the ballot of the
//                       survivors.  Dots stay implicit as (atom, k): mask u64 [T, words], cnt i32 [T]
//   k_depth_components  one workgroup per complex: exclusive scan of cnt, the accessible dots written in dot-id order
//                       (position, id, label = own index), then sweeps to the fixed point: a wave per atom with dots
//                       scans the atoms for those whose dots may link, lanes over their dots e take the minimum label
//                       of the linked dots of the atom, lower label[e] and hook e's former label below it (integer
//                       atomic minimum), then every dot jumps to the label of its label.  A label only ever takes the
//                       index of a dot of its own component, and the sweeps end when one lowers nothing: every label is
//                       then the smallest index of its component, whatever the order of the lanes was.  Sizes by integer
//                       atomics, the arg-max as one 64-bit key (size, -index)
//   k_depth_residues    one workgroup per target residue: atom after atom, the lanes take the minimum d^2 over the kept
//                       dots of the complex (a minimum of fp64 values: no order), one lane sums and takes the mean
// No floating-point atomics; a residue's bits depend on its complex alone: not on the batch, the chunk, the target list,
// the place in the grid or the run.
// Caps: DP_DOTS_CAP dots per atom; a complex of more than DP_CX_DOTS_CAP (atoms x n_dots) sets bit 0 of *status and its
// targets become NaN: never a wrong depth.
// Host emulation (DRGNN_EMU): a "wave" is one lane.
#pragma once
#include "drgnn_rt.h"

#define DP_DOTS_CAP 4096             // dots per atom
#define DP_CX_DOTS_CAP 4194304       // atoms x n_dots of one complex (its region of the workspace; 21 845 atoms at 192)
#define DP_MAX_GRID 4194303          // workgroups of one launch
#define DP_BAD -2                    // cx_outer of a complex beyond the cap

struct DepthArgs {
    const float* xyz;                // [T, 3]
    const int32_t* atom_ptr;         // [R + 1]
    const int32_t* res_ptr;          // [M + 1]
    const double* rad;               // [n_radii]
    const double* dots;              // [n_dots, 3]
    const int32_t* tgt_res;          // [K]
    const int32_t* tgt_cx;           // [K]
    int n_atoms, n_cx, n_radii, n_dots, words, all;
    double probe, link, link2;
    // workspace; the dots of a complex whose first atom is a0 live at [a0 n_dots, ..) of pos / id / label / size
    unsigned long long* mask;        // [T, words]
    double* pos;                     // [T n_dots, 3]
    int32_t* id;                     // [T n_dots] (atom - a0) n_dots + k, ascending
    int32_t* label;                  // [T n_dots] index (within the complex) of the first dot of the component
    int32_t* size;                   // [T n_dots] dots of the component, at its label
    int32_t* cnt;                    // [T] accessible dots of the atom
    int32_t* ptr;                    // [T] index of its first dot within the complex
    int32_t* cx_nd;                  // [M] accessible dots
    int32_t* cx_outer;               // [M] label kept, -1: all (or none to choose from), DP_BAD: refused
    double* out;                     // [K]
    int32_t* status;                 // [1]
};

struct DepthShared {
    int part[DRGNN_NTHREADS + 1];
    double red[DRGNN_NWAVES];
    double sum;
    long long best;
    int changed;
};

#ifdef DRGNN_EMU
#define DP_LANES 1
#define DP_NWAVES 1
#define DP_WAVE 0
#define DP_LANE 0
#define DP_BALLOT(p) ((p) ? 1ull : 0ull)
#define DP_NOFMA
#define DP_LOAD(p) (*(p))
DEV int dp_atomic_min(int32_t* p, int32_t v) { const int o = *p; if (v < o) *p = v; return o; }
DEV double dp_wave_min(double v) { return v; }
#else
#define DP_LANES DRGNN_WAVE
#define DP_NWAVES DRGNN_NWAVES
#define DP_WAVE ((int)threadIdx.x / DRGNN_WAVE)
#define DP_LANE ((int)threadIdx.x % DRGNN_WAVE)
#define DP_BALLOT(p) ((unsigned long long)__ballot(p))
#define DP_NOFMA _Pragma("clang fp contract(off)")
// labels are read and lowered while other waves lower them: every access goes to the device-coherent level
#define DP_LOAD(p) __hip_atomic_load((p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
DEV int dp_atomic_min(int32_t* p, int32_t v) { return atomicMin(p, v); }
DEV double dp_wave_min(double v) {
#pragma unroll
    for (int o = DRGNN_WAVE / 2; o > 0; o >>= 1) {
        const double w = __shfl_xor(v, o, DRGNN_WAVE);
        v = w < v ? w : v;
    }
    return v;
}
#endif

struct DpVec { double x, y, z; };
DEV DpVec dp_atom(const DepthArgs& a, int t) {
    const float* p = a.xyz + 3 * (int64_t)t;
    return DpVec{(double)p[0], (double)p[1], (double)p[2]};
}
DEV double dp_d2(DpVec a, DpVec b) {
    DP_NOFMA
    const double dx = a.x - b.x, dy = a.y - b.y, dz = a.z - b.z;
    return (dx * dx + dy * dy) + dz * dz;
}
DEV DpVec dp_dot(const DepthArgs& a, DpVec x, double R, int k) {
    DP_NOFMA
    const double* s = a.dots + 3 * (int64_t)k;
    return DpVec{x.x + R * s[0], x.y + R * s[1], x.z + R * s[2]};
}
DEV int dp_ctz(unsigned long long m) { return __builtin_ctzll(m); }
DEV int dp_popc(unsigned long long m) { return __builtin_popcountll(m); }
// the complex of atom t: the last c whose first atom is <= t and that holds atoms
DEV int dp_complex_of(const DepthArgs& a, int t) {
    int lo = 0, hi = a.n_cx - 1;                                     // the smallest c with first_atom(c + 1) > t
    while (lo < hi) {
        const int mid = (lo + hi) / 2;
        if (a.atom_ptr[a.res_ptr[mid + 1]] > t) hi = mid; else lo = mid + 1;
    }
    return lo;
}
DEV bool dp_refused(const DepthArgs& a, int na) { return (int64_t)na * a.n_dots > DP_CX_DOTS_CAP; }

// ---- k_depth_dots: the wave of atom t
DEV void depth_dots_atom(const DepthArgs& a, int t, int lane) {
    DP_NOFMA
    const int c = dp_complex_of(a, t);
    const int a0 = a.atom_ptr[a.res_ptr[c]], a1 = a.atom_ptr[a.res_ptr[c + 1]];
    if (dp_refused(a, a1 - a0)) return;
    const double ri = a.rad[t % a.n_radii];
    const double Ri = ri + a.probe;
    const DpVec xi = dp_atom(a, t);
    const int na = a1 - a0, chunks = (na + DP_LANES - 1) / DP_LANES;
    int total = 0;
    for (int w = 0; w < a.words; ++w) {
        unsigned long long word = 0;
        for (int kb = 0; kb < 64; kb += DP_LANES) {                  // (one trip on the device: a lane per dot of the word)
            const int k = w * 64 + kb + lane;
            bool acc = k < a.n_dots && ri > 0.0;
            const DpVec p = dp_dot(a, xi, Ri, acc ? k : 0);
            if (DP_BALLOT(acc)) {
                // the atoms in chunks around t: +0, +1, -1, +2, .. (bonded atoms sit next to t in the input, and a word
                // whose dots are all buried ends the scan); the chunks wrap around the complex and cover it
                for (int q = 0; q < chunks; ++q) {
                    const int o = (q & 1) ? (q + 1) / 2 : -(q / 2);
                    const int j0 = a0 + (((t - a0 - DP_LANES / 2 + o * DP_LANES) % na) + na) % na;
                    const int j = a0 + (j0 - a0 + lane) % na;                   // (fewer atoms than lanes: an atom is met twice)
                    bool near = false;
                    if (j != t) {
                        const double rj = a.rad[j % a.n_radii];
                        if (rj > 0.0) {
                            const double s = (Ri + (rj + a.probe)) * 1.001;
                            near = dp_d2(dp_atom(a, j), xi) <= s * s;
                        }
                    }
                    unsigned long long bits = DP_BALLOT(near);
                    while (bits) {
                        const int b = dp_ctz(bits);
                        const int jj = a0 + (j0 - a0 + b) % na;
                        bits &= bits - 1;
                        const double Rj = a.rad[jj % a.n_radii] + a.probe;
                        acc = acc && dp_d2(p, dp_atom(a, jj)) >= Rj * Rj;
                    }
                    if (!DP_BALLOT(acc)) break;
                }
            }
            word |= DP_BALLOT(acc) << kb;
        }
        if (lane == 0) a.mask[(int64_t)t * a.words + w] = word;
        total += dp_popc(word);
    }
    if (lane == 0) a.cnt[t] = total;
}

DEV void depth_dots_tile(const DepthArgs& a, int64_t tile) {
    const int64_t t = tile * DP_NWAVES + DP_WAVE;
    if (t < a.n_atoms) depth_dots_atom(a, (int)t, DP_LANE);
}

// ---- k_depth_components: the workgroup of complex c
DEV void depth_components(const DepthArgs& a, int c, DepthShared& s) {
    DP_NOFMA
    const int a0 = a.atom_ptr[a.res_ptr[c]], na = a.atom_ptr[a.res_ptr[c + 1]] - a0;
    if (dp_refused(a, na)) {
        FOR_TID(j, 1) { a.cx_nd[c] = 0; a.cx_outer[c] = DP_BAD; ATOMIC_OR(a.status, 1); }
        return;
    }
    const int64_t base = (int64_t)a0 * a.n_dots;
    double* pos = a.pos + 3 * base;
    int32_t *id = a.id + base, *label = a.label + base, *size = a.size + base;
    const int32_t* cnt = a.cnt + a0;
    int32_t* ptr = a.ptr + a0;
    FOR_TID(i, na) ptr[i] = cnt[i];
    FOR_TID(j, 1) { s.best = -1; s.changed = 0; }
    BARRIER();
    const int nd = wg_exscan(ptr, na, s.part);
    BARRIER();
    FOR_TID(i, na) {
        if (cnt[i] == 0) continue;
        const DpVec xi = dp_atom(a, a0 + i);
        const double Ri = a.rad[(a0 + i) % a.n_radii] + a.probe;
        int d = ptr[i];
        for (int w = 0; w < a.words; ++w) {
            unsigned long long m = a.mask[(int64_t)(a0 + i) * a.words + w];
            while (m) {
                const int k = w * 64 + dp_ctz(m);
                m &= m - 1;
                const DpVec p = dp_dot(a, xi, Ri, k);
                pos[3 * (int64_t)d] = p.x; pos[3 * (int64_t)d + 1] = p.y; pos[3 * (int64_t)d + 2] = p.z;
                id[d] = i * a.n_dots + k;
                label[d] = d;
                size[d] = 0;
                ++d;
            }
        }
    }
    BARRIER();
    const int wave = DP_WAVE, lane = DP_LANE;
    for (;;) {
        // ---- push: every atom lowers the labels of the dots linked to its own
        for (int i = wave; i < na; i += DP_NWAVES) {
            if (cnt[i] == 0) continue;
            const DpVec xi = dp_atom(a, a0 + i);
            const double Ri = a.rad[(a0 + i) % a.n_radii] + a.probe;
            const int d0 = ptr[i], d1 = d0 + cnt[i];
            for (int j0 = 0; j0 < na; j0 += DP_LANES) {
                const int j = j0 + lane;
                bool near = false;
                if (j < na && cnt[j] > 0) {
                    const double reach = ((Ri + (a.rad[(a0 + j) % a.n_radii] + a.probe)) + a.link) * 1.001;
                    near = dp_d2(dp_atom(a, a0 + j), xi) <= reach * reach;
                }
                unsigned long long bits = DP_BALLOT(near);
                while (bits) {
                    const int jj = j0 + dp_ctz(bits);
                    bits &= bits - 1;
                    const int e1 = ptr[jj] + cnt[jj];
                    for (int e = ptr[jj] + lane; e < e1; e += DP_LANES) {
                        const DpVec pe = DpVec{pos[3 * (int64_t)e], pos[3 * (int64_t)e + 1], pos[3 * (int64_t)e + 2]};
                        const int le = DP_LOAD(label + e);
                        int m = le;
                        for (int d = d0; d < d1; ++d) {
                            if (d == e) continue;
                            const DpVec pd = DpVec{pos[3 * (int64_t)d], pos[3 * (int64_t)d + 1], pos[3 * (int64_t)d + 2]};
                            if (dp_d2(pd, pe) <= a.link2) {
                                const int ld = DP_LOAD(label + d);
                                m = ld < m ? ld : m;
                            }
                        }
                        if (m < le) {
                            dp_atomic_min(label + e, m);
                            dp_atomic_min(label + le, m);
                            s.changed = 1;
                        }
                    }
                }
            }
        }
        BARRIER();
        // ---- jump: every dot takes the label of its label
        FOR_TID(d, nd) {
            int l = DP_LOAD(label + d);
            for (;;) {
                const int ll = DP_LOAD(label + l);
                if (ll >= l) break;
                l = ll;
            }
            dp_atomic_min(label + d, l);
        }
        BARRIER();
        const int again = s.changed;
        BARRIER();
        if (!again) break;
        FOR_TID(j, 1) s.changed = 0;
        BARRIER();
    }
    // ---- sizes and the component kept
    FOR_TID(d, nd) ATOMIC_ADD(size + DP_LOAD(label + d), 1);
    BARRIER();
    FOR_TID(d, nd) {
        if (DP_LOAD(label + d) == d) {
            const long long key = ((long long)DP_LOAD(size + d) << 32) | (long long)(unsigned)(INT_MAX - d);
            ATOMIC_MAX64(&s.best, key);
        }
    }
    BARRIER();
    FOR_TID(j, 1) {
        a.cx_nd[c] = nd;
        a.cx_outer[c] = (a.all || nd == 0) ? -1 : INT_MAX - (int)(unsigned)(s.best & 0xFFFFFFFFll);
    }
}

// ---- k_depth_residues: the workgroup of target k
DEV void depth_residue(const DepthArgs& a, int64_t k, DepthShared& s) {
    DP_NOFMA
    const int c = a.tgt_cx[k], r = a.tgt_res[k];
    const int outer = a.cx_outer[c], nd = a.cx_nd[c];
    if (outer == DP_BAD) {
        FOR_TID(j, 1) a.out[k] = __builtin_nan("");
        return;
    }
    const int64_t base = (int64_t)a.atom_ptr[a.res_ptr[c]] * a.n_dots;
    const double* pos = a.pos + 3 * base;
    const int32_t* label = a.label + base;
    const int t0 = a.atom_ptr[r], t1 = a.atom_ptr[r + 1];
    FOR_TID(j, 1) s.sum = 0.0;
    BARRIER();
    for (int t = t0; t < t1; ++t) {
        const DpVec x = dp_atom(a, t);
        double best = __builtin_inf();
#ifdef DRGNN_EMU
        for (int d = 0; d < nd; ++d) {
#else
        for (int d = (int)threadIdx.x; d < nd; d += DRGNN_NTHREADS) {
#endif
            if (outer >= 0 && label[d] != outer) continue;
            const double v = dp_d2(x, DpVec{pos[3 * (int64_t)d], pos[3 * (int64_t)d + 1], pos[3 * (int64_t)d + 2]});
            best = v < best ? v : best;
        }
        best = dp_wave_min(best);
        if (DP_LANE == 0) s.red[DP_WAVE] = best;
        BARRIER();
        FOR_TID(j, 1) {
            double m = s.red[0];
            for (int w = 1; w < DP_NWAVES; ++w) m = s.red[w] < m ? s.red[w] : m;
            s.sum = s.sum + (sqrt(m) - a.probe);
        }
        BARRIER();
    }
    FOR_TID(j, 1) a.out[k] = t1 > t0 ? s.sum / (double)(t1 - t0) : __builtin_nan("");
}
