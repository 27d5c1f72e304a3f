// drgnn_step_af.h -- which __global__ instance of the AGGREGATION-FIRST step families (drgnn_step2.h: sGAT / FoutNet;
// drgnn_step3.h: GINet) a launch takes.  The families are instantiated per padded feature width 16 / 32 / 48 / 64,
// {per-mini-batch, cached whole-set workspace}, {training, inference}; training launches of the 32- and 48-wide kernels also with the
// capacity-class LDS layout (CLS = 1, drgnn_step.h), the single-branch nets with one or two workgroups per graph.
//
// An instance is described by one key (AfKey); a UNIT is one (family, width): af_unit<FAM, W> maps a key to the address of one of
// the kernels of that unit, and thereby instantiates them.  In the library build (Makefile: DRGNN_SPLIT_TU) each unit is
// instantiated in a translation unit of its own (drgnn_step_tu.hip with -DDRGNN_AF_FAM=AF_<family> -DDRGNN_AF_W=<width>) and only
// declared everywhere else, so the kernels are compiled once, in parallel, and no list of them has to be kept in two places; a
// single-unit build (profiling / ablation variants) instantiates all of them in drgnn_capi.hip, at af_kernel's table.
#ifndef DRGNN_STEP_AF_H
#define DRGNN_STEP_AF_H
#ifndef DRGNN_EMU

// The families -- the one table of them: the Makefile names a unit's objects by these names and gives the optimisation levels.
//   GINET_TWO     k_step3_co_topo: one workgroup per (graph, branch)
//   GINET_ONE     k_step3b_co_topo: both branches of a graph in one workgroup
//   GINET_SG      k_step3b_co_topo<., ., 0, ., true>: S rows read from memory (graphs beyond the staged form's LDS)
//   SGAT, FOUT    k_step2_co_topo<DRGNN_SGAT / DRGNN_FOUT>
//   SGAT_WHOLE    k_step2_co_topo<DRGNN_SGAT, ., false, ., 1, true>: a unit of its own, see af_unit
//   SGAT_XG, FOUT_XG  k_step2_co_topo<., ., ., 0, ., ., 1 / 2>: x rows (level 2: S rows too) read from memory
//   GINET_ENS, SGAT_ENS, FOUT_ENS           k_step3b_ens / k_step2_ens: ensemble inference (K models per launch)
//   GINET_COHORT, SGAT_COHORT, FOUT_COHORT  k_step3b_cohort / k_step2_cohort: cohort training (K members per launch)
#define DRGNN_AF_FAMILIES(X)                                                                                            \
    X(GINET_TWO) X(GINET_ONE) X(GINET_SG) X(SGAT) X(FOUT) X(SGAT_WHOLE) X(SGAT_XG) X(FOUT_XG) X(GINET_ENS) X(SGAT_ENS) \
    X(FOUT_ENS) X(GINET_COHORT) X(SGAT_COHORT) X(FOUT_COHORT)
#define DRGNN_AF_ENUM(F) AF_##F,
enum AfFamily { DRGNN_AF_FAMILIES(DRGNN_AF_ENUM) AF_N_FAMILIES };
#undef DRGNN_AF_ENUM
constexpr int af_family_kind(int fam) {
    return (fam == AF_SGAT || fam == AF_SGAT_WHOLE || fam == AF_SGAT_XG || fam == AF_SGAT_ENS || fam == AF_SGAT_COHORT) ? DRGNN_SGAT
           : (fam == AF_FOUT || fam == AF_FOUT_XG || fam == AF_FOUT_ENS || fam == AF_FOUT_COHORT) ? DRGNN_FOUT
           : DRGNN_GINET;
}

enum { AF_AXIS_NONE, AF_AXIS_ENS, AF_AXIS_COHORT };
// cls: 1 = capacity-class layout, honoured for the 32- and 48-wide kernels only, training and inference launches -- the host
//      asks for nothing else; 48: the feature count of the reference's shipped regression models
// wgs: workgroups per graph (GINet 2: k_step3_co_topo; single-branch nets 2: the split layout, training launches only)
// level: the from-memory form.  GINet, one workgroup per graph: 1 = S from memory; sGAT / FoutNet: 1 / 2 = the from-memory levels
// axis: the member axis (the ensemble's models, the cohort's members); those kernels are the one-workgroup forms, gathered
struct AfKey {
    int kind, width;
    int wgs, level, cls;
    bool gather, train;
    int axis;
};

// (the instances of one kernel form for both settings of GATHER)
template <int XF, int CLS, bool TRAIN> const void* af_k3(bool gather) {
    return gather ? (const void*)k_step3_co_topo<XF, true, CLS, TRAIN> : (const void*)k_step3_co_topo<XF, false, CLS, TRAIN>;
}
template <int XF, int CLS, bool TRAIN, bool SG = false> const void* af_k3b(bool gather) {
    return gather ? (const void*)k_step3b_co_topo<XF, true, CLS, TRAIN, SG> : (const void*)k_step3b_co_topo<XF, false, CLS, TRAIN, SG>;
}
template <int KIND, int XF, int CLS, int SPLIT, bool TRAIN, int XG = 0> const void* af_k2(bool gather) {
    return gather ? (const void*)k_step2_co_topo<KIND, XF, true, CLS, SPLIT, TRAIN, XG>
                  : (const void*)k_step2_co_topo<KIND, XF, false, CLS, SPLIT, TRAIN, XG>;
}
// the from-memory forms (run-time LDS layout only): graphs whose S AND x tiles do not fit the 160 KiB -- level 1: the x rows
// stay in memory; level 2 (32-, 48- and 64-wide: the widths whose S tile fills the LDS before the edge arrays do): the S rows too
template <int KIND, int XF, int LV> const void* af_k2_level(const AfKey& k) {
    if (!k.train) return af_k2<KIND, XF, 0, 1, false, LV>(k.gather);
    return k.wgs == 2 ? af_k2<KIND, XF, 0, 2, true, LV>(k.gather) : af_k2<KIND, XF, 0, 1, true, LV>(k.gather);
}

// The kernel of unit (FAM, W) that key k asks for (af_kernel below has chosen the unit); nullptr: no such instance.
template <int FAM, int W> const void* af_unit(const AfKey& k) {
    constexpr int KIND = af_family_kind(FAM);
    constexpr int C1 = (W == 32 || W == 48) ? 1 : 0;
    const bool g = k.gather, c = k.cls && C1;
    if constexpr (FAM == AF_GINET_TWO) {
        if (!k.train) return c ? af_k3<W, C1, false>(g) : af_k3<W, 0, false>(g);
        return c ? af_k3<W, C1, true>(g) : af_k3<W, 0, true>(g);
    } else if constexpr (FAM == AF_GINET_ONE) {
        if (!k.train) return c ? af_k3b<W, C1, false>(g) : af_k3b<W, 0, false>(g);
        return c ? af_k3b<W, C1, true>(g) : af_k3b<W, 0, true>(g);
    } else if constexpr (FAM == AF_GINET_SG) {
        return k.train ? af_k3b<W, 0, true, true>(g) : af_k3b<W, 0, false, true>(g);
    } else if constexpr (FAM == AF_SGAT || FAM == AF_FOUT) {
        // (split: two workgroups per graph, training launches only)
        if (!k.train) return c ? af_k2<KIND, W, C1, 1, false>(g) : af_k2<KIND, W, 0, 1, false>(g);
        if (k.wgs == 2) return c ? af_k2<KIND, W, C1, 2, true>(g) : af_k2<KIND, W, 0, 2, true>(g);
        if constexpr (FAM == AF_FOUT) {
            return c ? af_k2<KIND, W, C1, 1, true>(g) : af_k2<KIND, W, 0, 1, true>(g);
        } else {
            if (!g) return nullptr;      // (AF_SGAT_WHOLE's)
            return c ? (const void*)k_step2_co_topo<KIND, W, true, C1, 1, true> : (const void*)k_step2_co_topo<KIND, W, true, 0, 1, true>;
        }
    } else if constexpr (FAM == AF_SGAT_WHOLE) {
        // sGAT's training launches with one workgroup per graph on a per-mini-batch workspace are the ones whose co-launched
        // builder -- one workgroup per graph working BOTH chains off, with edge weights -- bounds the launch (batch 128 and
        // beyond, topology rebuilt).  The single-branch units are compiled at -Os (Makefile), which suits the step's phases and
        // costs that builder chain 1 us (profiles/r05_ab_opt_level.txt): these instances live in a unit of their own, compiled
        // at -O3.
        // (48 features: the class instance of THIS launch is slower than the run-time layout -- 27.45 against 26.77 us per step
        // at batch 128, profiles/r05_cls48_ab.txt -- although it does not spill: the run-time layout with the class's capacities
        // steps those)
        constexpr int CW = (W == 32) ? 1 : 0;
        if (k.cls && CW) return (const void*)k_step2_co_topo<DRGNN_SGAT, W, false, CW, 1, true>;
        return (const void*)k_step2_co_topo<DRGNN_SGAT, W, false, 0, 1, true>;
    } else if constexpr (FAM == AF_SGAT_XG || FAM == AF_FOUT_XG) {
        if constexpr (W >= 32) { if (k.level == 2) return af_k2_level<KIND, W, 2>(k); }
        return k.level == 1 ? af_k2_level<KIND, W, 1>(k) : nullptr;
    } else if constexpr (FAM == AF_GINET_ENS) {
        // the ensemble instances (drgnn_kernels.h: k_step3b_ens / k_step2_ens): the inference instances of the one-workgroup
        // forms a single-model launch takes, with a model axis
        if (k.level) return (const void*)k_step3b_ens<W, 0, true>;
        return c ? (const void*)k_step3b_ens<W, C1, false> : (const void*)k_step3b_ens<W, 0, false>;
    } else if constexpr (FAM == AF_SGAT_ENS || FAM == AF_FOUT_ENS) {
        if (k.level == 1) return (const void*)k_step2_ens<KIND, W, 0, 1>;
        if constexpr (W >= 32) { if (k.level == 2) return (const void*)k_step2_ens<KIND, W, 0, 2>; }
        if (k.level) return nullptr;
        return c ? (const void*)k_step2_ens<KIND, W, C1, 0> : (const void*)k_step2_ens<KIND, W, 0, 0>;
    } else if constexpr (FAM == AF_GINET_COHORT) {
        // the cohort instances (drgnn_kernels.h: k_step3b_cohort / k_step2_cohort): the TRAINING instances of the same forms,
        // with a member axis; same classes and from-memory levels as the ensemble's
        if (k.level) return (const void*)k_step3b_cohort<W, 0, true>;
        return c ? (const void*)k_step3b_cohort<W, C1, false> : (const void*)k_step3b_cohort<W, 0, false>;
    } else {
        static_assert(FAM == AF_SGAT_COHORT || FAM == AF_FOUT_COHORT, "DRGNN_AF_FAM: one of DRGNN_AF_FAMILIES");
        if (k.level == 1) return (const void*)k_step2_cohort<KIND, W, 0, 1>;
        if constexpr (W >= 32) { if (k.level == 2) return (const void*)k_step2_cohort<KIND, W, 0, 2>; }
        if (k.level) return nullptr;
        return c ? (const void*)k_step2_cohort<KIND, W, C1, 0> : (const void*)k_step2_cohort<KIND, W, 0, 0>;
    }
}

#define DRGNN_AF_WIDTHS(X, F) X(F, 16) X(F, 32) X(F, 48) X(F, 64)
#if defined(DRGNN_SPLIT_TU)
#define DRGNN_AF_EXTERN_1(F, W) extern template const void* af_unit<AF_##F, W>(const AfKey&);
#define DRGNN_AF_EXTERN(F) DRGNN_AF_WIDTHS(DRGNN_AF_EXTERN_1, F)
DRGNN_AF_FAMILIES(DRGNN_AF_EXTERN)
#undef DRGNN_AF_EXTERN
#undef DRGNN_AF_EXTERN_1
#endif

#if defined(DRGNN_KERNELS_MAIN)
// From key to unit, the one dispatcher.  nullptr: no such instance.
static const void* af_kernel(const AfKey& k) {
    typedef const void* (*af_unit_fn)(const AfKey&);
#define DRGNN_AF_ENTRY(F, W) af_unit<AF_##F, W>,
#define DRGNN_AF_ROW(F) {DRGNN_AF_WIDTHS(DRGNN_AF_ENTRY, F)},
    static const af_unit_fn units[AF_N_FAMILIES][4] = {DRGNN_AF_FAMILIES(DRGNN_AF_ROW)};
#undef DRGNN_AF_ROW
#undef DRGNN_AF_ENTRY
    if (k.width != 16 && k.width != 32 && k.width != 48 && k.width != 64) return nullptr;
    const bool ginet = k.kind == DRGNN_GINET, sgat = k.kind == DRGNN_SGAT;
    int fam;
    if (k.axis == AF_AXIS_ENS) fam = ginet ? AF_GINET_ENS : sgat ? AF_SGAT_ENS : AF_FOUT_ENS;
    else if (k.axis == AF_AXIS_COHORT) fam = ginet ? AF_GINET_COHORT : sgat ? AF_SGAT_COHORT : AF_FOUT_COHORT;
    else if (ginet) fam = k.wgs == 2 ? AF_GINET_TWO : k.level ? AF_GINET_SG : AF_GINET_ONE;
    else if (k.level) fam = sgat ? AF_SGAT_XG : AF_FOUT_XG;
    // (sGAT, training, one workgroup per graph, not gathered: the unit compiled at -O3, see af_unit)
    else if (sgat && k.train && k.wgs != 2 && !k.gather) fam = AF_SGAT_WHOLE;
    else fam = sgat ? AF_SGAT : AF_FOUT;
    return units[fam][k.width / 16 - 1](k);
}
#endif  // DRGNN_KERNELS_MAIN

#endif  // !DRGNN_EMU
#endif
