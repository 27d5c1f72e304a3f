// drgnn_metrics.h -- evaluation scores of a test set (the reference's Metrics, Metrics.py): confusion counts, the
// regression sums, a stable LSD radix sort (ranking by prediction, median of |y - pred|) and the hit-rate scan.
//
// Every value is float64 on the device.  Integer results are int64; no floating-point atomics anywhere and every
// floating-point combination runs in a fixed order, so the results are bit-identical from launch to launch.
//
// Kernels (all 256-lane workgroups except the one-workgroup scans, MT_SNT lanes):
//   k_mt_reduce   per-workgroup partials of the first read of (pred, y): confusion counts, non-finite / non-integral
//                 counts, min(y), min(pred), sum y, sum r, sum |r|, sum r^2, max |r|, sum (log1p y - log1p p)^2
//                 (r = y - pred); with centred = 1 the second read: sum (y - ybar)^2, sum (r - rbar)^2
//   k_mt_combine  one workgroup: the partials in workgroup order
//   k_mt_keys     order-preserving 64-bit keys of pred (payload: 0..n-1) or of |r| (no payload)
//   k_mt_hist / k_mt_scan / k_mt_scatter   one 8-bit digit of the LSD sort: per-tile histogram (digit-major),
//                 exclusive scan over (digit, tile) in one workgroup, stable scatter (ranks in original order)
//   k_mt_median   one lane: the median of the sorted |r|
//   k_mt_hit_tiles / k_mt_hit_scan / k_mt_hit_write   gt[idx] gathered in rank order, multi-tile inclusive scan into
//                 int64 [n]; the AUC sum S = sum over positives i of idx[i] in the same first read
// No workgroup waits on another: each step is its own launch, so the emulation (workgroups one after another) and
// the device run the same phases.
#pragma once
#include "drgnn_rt.h"

#define MT_NT 256                       // lanes of the tiled / reduction kernels
#define MT_SNT 1024                     // lanes of the one-workgroup scans
#define MT_ITEMS 16                     // keys per lane per radix / hit-rate tile
#define MT_TILE (MT_NT * MT_ITEMS)      // 4096
#define MT_RADIX 256
#define MT_PASSES 8                     // 64-bit keys, 8-bit digits
#define MT_RED_WGS 512                  // most workgroups of a reduction pass
#define MT_KMAX 8                       // most labels of the confusion matrix
#define MT_NF 16                        // doubles per reduction partial
#define MT_NI (3 + MT_KMAX * MT_KMAX)   // int64 per reduction partial: nonfinite, nonintegral, y in labels, K x K

// slots of the int64 result (drgnn_metrics' counts) and of the float64 result (scores)
enum { MT_C_NONFINITE = 0, MT_C_NONINTEGRAL = 1, MT_C_YIN = 2, MT_C_POS = 3, MT_C_AUCSUM = 4, MT_C_CONF = 8 };
enum { MT_S_MINY = 0, MT_S_MINP, MT_S_SUMY, MT_S_SUMR, MT_S_SUMABS, MT_S_SUMSQ, MT_S_MAXABS, MT_S_SUMLOG,
       MT_S_CY2, MT_S_CR2, MT_S_MEDIAN, MT_S_COUNT };

// one lane's body of a phase: every lane on the device, lanes 0..NT-1 in order in the emulation
#ifdef DRGNN_EMU
#define MT_LANES(t, NT) for (int t = 0; t < (NT); ++t)
#else
#define MT_LANES(t, NT) for (int t = (int)threadIdx.x, t##_once = 1; t##_once; t##_once = 0)
#endif

struct MetricsArgs {
    const double* pred;
    const double* y;
    int64_t n;
    double thr;
    int dir;               // +1: positive means x > thr (fnat, bin_class); -1: x < thr
    int lo, K;             // K = 0: binarise both vectors (labels {0, 1}); else labels lo .. lo + K - 1 as they are
    int G;                 // reduction workgroups
    int n_tiles;           // radix / hit-rate tiles of MT_TILE
    double* fpart;         // [G][MT_NF]
    long long* ipart;      // [G][MT_NI]
    unsigned long long* keys[2];
    int32_t* vals[2];      // vals[0]: the caller's order buffer (ranking), null for the |r| sort
    int32_t* hist;         // [MT_RADIX][n_tiles], scanned in place
    long long* tsum;       // [n_tiles] hits per tile, scanned in place
    long long* ssum;       // [n_tiles] AUC sum per tile
    long long* counts;     // result (MT_C_*)
    double* scores;        // result (MT_S_*)
    long long* hits;       // [n] hit-rate
};

DEV unsigned long long mt_bits(double v) {
#ifdef DRGNN_EMU
    unsigned long long u;
    memcpy(&u, &v, 8);
    return u;
#else
    return (unsigned long long)__double_as_longlong(v);
#endif
}
DEV double mt_double(unsigned long long u) {
#ifdef DRGNN_EMU
    double v;
    memcpy(&v, &u, 8);
    return v;
#else
    return __longlong_as_double((long long)u);
#endif
}
// ascending order of doubles as unsigned order of keys; -0 is +0 (a tie, as numpy has it), NaN sorts last
DEV unsigned long long mt_key(double v) {
    if (v != v) return ~0ull;
    if (v == 0.0) v = 0.0;
    const unsigned long long u = mt_bits(v);
    return (u >> 63) ? ~u : (u | (1ull << 63));
}
DEV double mt_unkey(unsigned long long k) { return mt_double((k >> 63) ? (k ^ (1ull << 63)) : ~k); }

DEV int mt_positive(double v, const MetricsArgs& a) { return a.dir > 0 ? (v > a.thr) : (v < a.thr); }
// confusion row / column of a value, -1 outside the labels (ignored, as sklearn's confusion_matrix does)
DEV int mt_class(double v, const MetricsArgs& a) {
    if (a.K == 0) return mt_positive(v, a);
    if (!(v == floor(v)) || v < (double)a.lo || v > (double)(a.lo + a.K - 1)) return -1;
    return (int)v - a.lo;
}
DEV bool mt_finite(double v) { return v == v && v - v == 0.0; }

// ---- reductions --------------------------------------------------------------------------------------------------
struct MtRedShared {
    double f[8][MT_NT];
    long long c[3][MT_NT];
    long long conf[MT_KMAX * MT_KMAX];
};

// workgroup g of the first (centred = 0) or second (centred = 1) read
DEV void mt_reduce_block(const MetricsArgs& a, int g, int centred, MtRedShared& s) {
    const int KK = (a.K == 0 ? 2 : a.K) * (a.K == 0 ? 2 : a.K);
    MT_LANES(t, MT_NT) {
        if (t < KK) s.conf[t] = 0;
    }
    BARRIER();
    const int64_t stride = (int64_t)a.G * MT_NT;
    MT_LANES(t, MT_NT) {
        double f[8];
        long long c[3] = {0, 0, 0};
        if (!centred) {
            f[0] = INFINITY; f[1] = INFINITY; f[2] = 0; f[3] = 0; f[4] = 0; f[5] = 0; f[6] = 0; f[7] = 0;
            const int Kc = a.K == 0 ? 2 : a.K;
            for (int64_t i = (int64_t)g * MT_NT + t; i < a.n; i += stride) {
                const double y = a.y[i], p = a.pred[i];
                const bool fin = mt_finite(y) && mt_finite(p);
                c[0] += !fin;
                c[1] += (mt_finite(y) && y != floor(y)) || (mt_finite(p) && p != floor(p));
                const int cy = mt_class(y, a), cp = mt_class(p, a);
                c[2] += cy >= 0;
                if (cy >= 0 && cp >= 0) ATOMIC_ADD64(&s.conf[cy * Kc + cp], 1);
                const double r = y - p, ar = fabs(r), lg = log1p(y) - log1p(p);
                f[0] = fmin(f[0], y);
                f[1] = fmin(f[1], p);
                f[2] += y;
                f[3] += r;
                f[4] += ar;
                f[5] += r * r;
                f[6] = ar > f[6] || ar != ar ? ar : f[6];
                f[7] += lg * lg;
            }
        } else {
            const double ybar = a.scores[MT_S_SUMY] / (double)a.n, rbar = a.scores[MT_S_SUMR] / (double)a.n;
            for (int j = 0; j < 8; ++j) f[j] = 0;
            for (int64_t i = (int64_t)g * MT_NT + t; i < a.n; i += stride) {
                const double y = a.y[i], dy = y - ybar, dr = (y - a.pred[i]) - rbar;
                f[0] += dy * dy;
                f[1] += dr * dr;
            }
        }
        for (int j = 0; j < 8; ++j) s.f[j][t] = f[j];
        for (int j = 0; j < 3; ++j) s.c[j][t] = c[j];
    }
    BARRIER();
    for (int h = MT_NT / 2; h > 0; h >>= 1) {
        MT_LANES(t, MT_NT) {
            if (t < h) {
                const int u = t + h;
                if (!centred) {
                    s.f[0][t] = fmin(s.f[0][t], s.f[0][u]);
                    s.f[1][t] = fmin(s.f[1][t], s.f[1][u]);
                    for (int j = 2; j < 6; ++j) s.f[j][t] += s.f[j][u];
                    const double m = s.f[6][u];
                    if (m > s.f[6][t] || m != m) s.f[6][t] = m;
                    s.f[7][t] += s.f[7][u];
                    for (int j = 0; j < 3; ++j) s.c[j][t] += s.c[j][u];
                } else {
                    s.f[0][t] += s.f[0][u];
                    s.f[1][t] += s.f[1][u];
                }
            }
        }
        BARRIER();
    }
    MT_LANES(t, MT_NT) {
        if (!centred) {
            if (t < 8) a.fpart[(int64_t)g * MT_NF + t] = s.f[t][0];
            if (t < 3) a.ipart[(int64_t)g * MT_NI + t] = s.c[t][0];
            if (t < KK) a.ipart[(int64_t)g * MT_NI + 3 + t] = s.conf[t];
        } else if (t < 2) {
            a.fpart[(int64_t)g * MT_NF + 8 + t] = s.f[t][0];
        }
    }
}

// one workgroup: lane q combines quantity q over the G partials in workgroup order
DEV void mt_combine_block(const MetricsArgs& a, int centred) {
    const int KK = (a.K == 0 ? 2 : a.K) * (a.K == 0 ? 2 : a.K);
    MT_LANES(t, MT_NT) {
        if (!centred && t < 8) {
            double v = (t < 2) ? INFINITY : 0.0;
            for (int g = 0; g < a.G; ++g) {
                const double x = a.fpart[(int64_t)g * MT_NF + t];
                if (t < 2) v = fmin(v, x);
                else if (t == 6) v = (x > v || x != x) ? x : v;
                else v += x;
            }
            a.scores[t] = v;
        } else if (centred && t < 2) {
            double v = 0.0;
            for (int g = 0; g < a.G; ++g) v += a.fpart[(int64_t)g * MT_NF + 8 + t];
            a.scores[MT_S_CY2 + t] = v;
        } else if (!centred && t >= 64 && t < 64 + 3 + KK) {
            const int q = t - 64;
            long long v = 0;
            for (int g = 0; g < a.G; ++g) v += a.ipart[(int64_t)g * MT_NI + q];
            a.counts[q < 3 ? q : MT_C_CONF + q - 3] = v;
        }
    }
}

// ---- LSD radix sort ----------------------------------------------------------------------------------------------
// keys of pred (payload 0..n-1 into vals[0]) or of |y - pred| (no payload)
DEV void mt_keys_block(const MetricsArgs& a, int tile, int absres) {
    MT_LANES(t, MT_NT) {
        for (int k = 0; k < MT_ITEMS; ++k) {
            const int64_t i = (int64_t)tile * MT_TILE + (int64_t)k * MT_NT + t;
            if (i < a.n) {
                a.keys[0][i] = mt_key(absres ? fabs(a.y[i] - a.pred[i]) : a.pred[i]);
                if (!absres) a.vals[0][i] = (int32_t)i;
            }
        }
    }
}

struct MtHistShared {
    int h[MT_RADIX];
};

DEV void mt_hist_block(const MetricsArgs& a, int tile, int pass, MtHistShared& s) {
    const unsigned long long* src = a.keys[pass & 1];
    const int sh = 8 * pass;
    MT_LANES(t, MT_NT) { s.h[t] = 0; }
    BARRIER();
    MT_LANES(t, MT_NT) {
        for (int k = 0; k < MT_ITEMS; ++k) {
            const int64_t i = (int64_t)tile * MT_TILE + (int64_t)k * MT_NT + t;
            if (i < a.n) ATOMIC_ADD(&s.h[(int)((src[i] >> sh) & 255)], 1);
        }
    }
    BARRIER();
    MT_LANES(t, MT_NT) { a.hist[(int64_t)t * a.n_tiles + tile] = s.h[t]; }
}

struct MtScanShared {
    long long part[MT_SNT];
};

// one workgroup: exclusive scan of v[0..m) in place (each lane a contiguous chunk); returns the total in part[0]
// after the last barrier
template <typename T>
DEV void mt_exscan_block(T* v, int64_t m, MtScanShared& s) {
    const int64_t chunk = (m + MT_SNT - 1) / MT_SNT;
    MT_LANES(t, MT_SNT) {
        const int64_t lo = (int64_t)t * chunk < m ? (int64_t)t * chunk : m;
        const int64_t hi = lo + chunk < m ? lo + chunk : m;
        long long sum = 0;
        for (int64_t i = lo; i < hi; ++i) sum += (long long)v[i];
        s.part[t] = sum;
    }
    BARRIER();
    MT_LANES(t, MT_SNT) {
        if (t == 0) {
            long long run = 0;
            for (int j = 0; j < MT_SNT; ++j) { const long long x = s.part[j]; s.part[j] = run; run += x; }
        }
    }
    BARRIER();
    MT_LANES(t, MT_SNT) {
        const int64_t lo = (int64_t)t * chunk < m ? (int64_t)t * chunk : m;
        const int64_t hi = lo + chunk < m ? lo + chunk : m;
        long long run = s.part[t];
        for (int64_t i = lo; i < hi; ++i) { const long long x = (long long)v[i]; v[i] = (T)run; run += x; }
    }
}

struct MtScatterShared {
    unsigned long long key[MT_NT];
    int val[MT_NT];
    int dig[MT_NT];
    int rank[MT_NT];
    int wcnt[MT_NT / DRGNN_WAVE][MT_RADIX];
    int wpre[MT_NT / DRGNN_WAVE][MT_RADIX];
    int run[MT_RADIX];
    int base[MT_RADIX];
};

// stable scatter of one tile for digit `pass`: item order inside the tile is (round, wave, lane), the original order
DEV void mt_scatter_block(const MetricsArgs& a, int tile, int pass, MtScatterShared& s) {
    const unsigned long long* src = a.keys[pass & 1];
    unsigned long long* dst = a.keys[(pass + 1) & 1];
    const int32_t* vsrc = a.vals[pass & 1];
    int32_t* vdst = a.vals[(pass + 1) & 1];
    const int sh = 8 * pass;
    MT_LANES(t, MT_NT) {
        s.run[t] = 0;
        s.base[t] = a.hist[(int64_t)t * a.n_tiles + tile];
        for (int w = 0; w < MT_NT / DRGNN_WAVE; ++w) s.wcnt[w][t] = 0;
    }
    BARRIER();
    for (int r = 0; r < MT_ITEMS; ++r) {
        MT_LANES(t, MT_NT) {
            const int64_t i = (int64_t)tile * MT_TILE + (int64_t)r * MT_NT + t;
            const bool valid = i < a.n;
            const unsigned long long key = valid ? src[i] : 0ull;
            const int d = (int)((key >> sh) & 255);
            s.key[t] = key;
            s.val[t] = (valid && vsrc) ? vsrc[i] : 0;
            s.dig[t] = valid ? d : -1;
            const int wave = t / DRGNN_WAVE, lane = t % DRGNN_WAVE;
#ifdef DRGNN_EMU
            int rank = 0;
            for (int l = t - lane; l < t; ++l) rank += s.dig[l] == d;
#else
            // lanes of this wave holding the same digit: eight ballots; the rank is the count of those before this lane
            unsigned long long same = __ballot(valid);
            for (int b = 0; b < 8; ++b) {
                const bool bit = (d >> b) & 1;
                const unsigned long long bal = __ballot(bit);
                same &= bit ? bal : ~bal;
            }
            const int rank = __popcll(same & ((1ull << lane) - 1ull));
#endif
            s.rank[t] = rank;
            if (valid) ATOMIC_ADD(&s.wcnt[wave][d], 1);
        }
        BARRIER();
        MT_LANES(t, MT_NT) {           // lane t: digit t
            int run = s.run[t];
            for (int w = 0; w < MT_NT / DRGNN_WAVE; ++w) {
                const int c = s.wcnt[w][t];
                s.wcnt[w][t] = 0;
                s.wpre[w][t] = run;
                run += c;
            }
            s.run[t] = run;
        }
        BARRIER();
        MT_LANES(t, MT_NT) {
            const int d = s.dig[t];
            if (d >= 0) {
                const int64_t o = (int64_t)s.base[d] + s.wpre[t / DRGNN_WAVE][d] + s.rank[t];
                if (o >= 0 && o < a.n) {
                    dst[o] = s.key[t];
                    if (vdst) vdst[o] = s.val[t];
                }
            }
        }
        BARRIER();
    }
}

// median of the sorted |r| (keys[0] after an even number of passes), as np.median takes it
DEV void mt_median(const MetricsArgs& a) {
    const int64_t h = a.n / 2;
    const double hi = mt_unkey(a.keys[0][h]);
    a.scores[MT_S_MEDIAN] = (a.n & 1) ? hi : (mt_unkey(a.keys[0][h - 1]) + hi) / 2.0;
}

// ---- hit rate and the AUC sum --------------------------------------------------------------------------------------
struct MtHitShared {
    long long h[MT_NT];
    long long s[MT_NT];
};

// position j of the ranking (ascending argsort, reversed for dir > 0)
DEV int32_t mt_idx(const MetricsArgs& a, int64_t j) { return a.vals[0][a.dir > 0 ? a.n - 1 - j : j]; }

// lane t holds positions tile * MT_TILE + t * MT_ITEMS + (0 .. MT_ITEMS): the hits among them and their AUC sum;
// write = 0: the tile's totals into tsum / ssum; write = 1: the inclusive scan into hits (tsum scanned already)
DEV void mt_hit_block(const MetricsArgs& a, int tile, int write, MtHitShared& s) {
    MT_LANES(t, MT_NT) {
        long long h = 0, sum = 0;
        for (int k = 0; k < MT_ITEMS; ++k) {
            const int64_t j = (int64_t)tile * MT_TILE + (int64_t)t * MT_ITEMS + k;
            if (j < a.n) {
                const int32_t idx = mt_idx(a, j);
                h += mt_positive(a.y[idx], a);
                if (!write && mt_positive(a.y[j], a)) sum += idx;
            }
        }
        s.h[t] = h;
        s.s[t] = sum;
    }
    BARRIER();
    if (!write) {
        for (int half = MT_NT / 2; half > 0; half >>= 1) {
            MT_LANES(t, MT_NT) {
                if (t < half) { s.h[t] += s.h[t + half]; s.s[t] += s.s[t + half]; }
            }
            BARRIER();
        }
        MT_LANES(t, MT_NT) {
            if (t == 0) { a.tsum[tile] = s.h[0]; a.ssum[tile] = s.s[0]; }
        }
        return;
    }
    MT_LANES(t, MT_NT) {
        if (t == 0) {
            long long run = a.tsum[tile];
            for (int j = 0; j < MT_NT; ++j) { const long long x = s.h[j]; s.h[j] = run; run += x; }
        }
    }
    BARRIER();
    MT_LANES(t, MT_NT) {
        long long run = s.h[t];
        for (int k = 0; k < MT_ITEMS; ++k) {
            const int64_t j = (int64_t)tile * MT_TILE + (int64_t)t * MT_ITEMS + k;
            if (j < a.n) {
                run += mt_positive(a.y[mt_idx(a, j)], a);
                a.hits[j] = run;
            }
        }
    }
}

// one workgroup: the tile totals scanned (exclusive, in place), P and S into counts
DEV void mt_hit_scan_block(const MetricsArgs& a, MtScanShared& s) {
    MT_LANES(t, MT_SNT) {
        if (t == 0) {
            long long p = 0, sum = 0;
            for (int i = 0; i < a.n_tiles; ++i) { p += a.tsum[i]; sum += a.ssum[i]; }
            a.counts[MT_C_POS] = p;
            a.counts[MT_C_AUCSUM] = sum;
        }
    }
    BARRIER();
    mt_exscan_block<long long>(a.tsum, a.n_tiles, s);
}

// ---- workspace ---------------------------------------------------------------------------------------------------
HD int64_t mt_align(int64_t b) { return (b + 255) & ~(int64_t)255; }
HD int64_t mt_tiles(int64_t n) { return (n + MT_TILE - 1) / MT_TILE; }
// byte offsets of keys0, keys1, vals1, hist, fpart, ipart, tsum, ssum; [8] = total
HD void mt_layout(int64_t n, int64_t* off) {
    const int64_t T = mt_tiles(n);
    const int64_t sz[8] = {8 * n, 8 * n, 4 * n, 4 * (int64_t)MT_RADIX * T, 8 * (int64_t)MT_NF * MT_RED_WGS,
                           8 * (int64_t)MT_NI * MT_RED_WGS, 8 * T, 8 * T};
    int64_t o = 0;
    for (int i = 0; i < 8; ++i) { off[i] = o; o += mt_align(sz[i]); }
    off[8] = o;
}
