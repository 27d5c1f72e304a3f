"""Interface graphs of complexes on the device: count and fill (csrc/drgnn_iface.h) into a ``GraphStore``, or packed on
the device (csrc/drgnn_pack.h) into a ``ResidentGraphSet``."""
import numpy as np
import torch

from . import _lib
from ._request import Request
from .atoms import RESIDUE_CHARGE, RESIDUE_POLARITY, _complexes, _default_device, _ragged
from .dock_scores import SCORE_KEYS, attach_scores, docking_scores, lddt_scores
from .residue_features import FEATURES, _feature_chunk

WORKSPACE_BUDGET = 256 << 20       # bytes of dense min-d^2 workspace one call may ask for (sets the default chunk)


def build_ragged_device(api, xyz, atom_ptr, res_ptr, res_split, res_type, contact_distance=8.5, internal_contact_distance=3.0,
                        device="cpu", tile_atoms=0, workspace_bytes=None):
    """One drgnn_iface_count + drgnn_iface_fill over a ragged batch given as numpy arrays (include/drgnn.h), the results
    left on ``device``: (out, ptrs) with ``out`` the dict of the eight outputs of drgnn_iface_fill as tensors and
    ``ptrs`` int32 [3, M+1] = node_ptr / edge_ptr / iedge_ptr.  Only the three totals come back to the host."""
    M, R = len(res_ptr) - 1, len(atom_ptr) - 1
    r = Request(_lib.IfaceRequest, device)
    dev = r.device
    d_xyz = r.input("xyz", xyz, torch.float32)
    r.table("atom_ptr", atom_ptr)
    rp, rs = r.table("res_ptr", res_ptr)[0].astype(np.int64), r.table("res_split", res_split)[0].astype(np.int64)
    r.input("res_type", res_type, torch.int32)
    if workspace_bytes is None:
        workspace_bytes = api.iface_workspace_bytes(M, int((rs - rp[:-1]).max()) if M else 0,
                                                    int((rp[1:] - rs).max()) if M else 0, R)
    r.output("workspace", max(int(workspace_bytes), 16), torch.uint8)
    ptrs = r.output(("node_ptr", "edge_ptr", "iedge_ptr"), (3, M + 1), torch.int32, zeros=True)
    r.set(n_atoms=int(d_xyz.shape[0]), n_residues=R, n_complexes=M, contact_distance=float(contact_distance),
          internal_contact_distance=float(internal_contact_distance), tile_atoms=int(tile_atoms),
          workspace_bytes=int(workspace_bytes))
    r.run(api, "iface_count")
    N, E, Ei = (int(v) for v in ptrs[:, -1].cpu())                 # the one synchronisation of the build
    out = {"node_residue": torch.empty(N, dtype=torch.int32, device=dev), "pos": torch.empty((N, 3), dtype=torch.float32, device=dev),
           "chain": torch.empty(N, dtype=torch.int32, device=dev), "type": torch.empty(N, dtype=torch.int32, device=dev),
           "edge_index": torch.empty((E, 2), dtype=torch.int64, device=dev), "dist": torch.empty(E, dtype=torch.float32, device=dev),
           "internal_edge_index": torch.empty((Ei, 2), dtype=torch.int64, device=dev),
           "internal_dist": torch.empty(Ei, dtype=torch.float32, device=dev)}
    api.iface_fill(r.q, N, E, Ei, out["node_residue"], out["pos"], out["chain"], out["type"], out["edge_index"], out["dist"],
                   out["internal_edge_index"], out["internal_dist"], r.stream())
    return out, ptrs


def build_ragged(api, xyz, atom_ptr, res_ptr, res_split, res_type, contact_distance=8.5, internal_contact_distance=3.0,
                 device="cpu", tile_atoms=0, workspace_bytes=None):
    """``build_ragged_device`` copied to the host.  Returns a dict of numpy arrays: node_ptr / edge_ptr / iedge_ptr int32
    [M+1] and the eight outputs of drgnn_iface_fill."""
    out, ptrs = build_ragged_device(api, xyz, atom_ptr, res_ptr, res_split, res_type, contact_distance,
                                    internal_contact_distance, device, tile_atoms, workspace_bytes)
    res = {k: v.cpu().numpy() for k, v in out.items()}
    p = ptrs.cpu().numpy()
    res["node_ptr"], res["edge_ptr"], res["iedge_ptr"] = p[0], p[1], p[2]
    return res


def default_chunk(api, max_res_a, max_res_b, max_atoms, budget=WORKSPACE_BUDGET):
    """the largest number of complexes of these bounds whose workspace stays within ``budget`` bytes (at least 1; the
    grid and the int32 offsets bound it too)"""
    lo, hi = 1, 65535
    hi = min(hi, max(1, (2 ** 31 - 1) // (3 * max(max_atoms, 1))))
    while lo < hi:
        mid = (lo + hi + 1) // 2
        if api.iface_workspace_bytes(mid, max_res_a, max_res_b, mid * (max_res_a + max_res_b)) <= budget:
            lo = mid
        else:
            hi = mid - 1
    return lo


def interface_graphs(tables_or_poses, names, contact_distance=8.5, internal_contact_distance=3.0, device=None, chunk=None,
                     api=None, reference=None, bsa=False, hse=False, depth=False, lddt=None):
    """Interface graphs of complexes (a sequence of ``AtomTable``, an ``AtomTable.poses`` batch, or a mix) as a
    ``GraphStore`` with one molecule per name, in the reference's tree: ``edge_index``, ``edge_data/dist``,
    ``internal_edge_index``, ``internal_edge_data/dist``, ``nodes`` and, under ``node_data/``, ``pos``, ``chain``,
    ``type`` (one-hot 20), ``polarity`` (one-hot 4), ``charge`` and ``residue`` (index into the table's residues).
    ``chunk``: complexes per kernel call, which bounds the dense workspace (default: what fits WORKSPACE_BUDGET
    bytes); it changes no bit of the result.  ``api`` / ``device``: the product library on the GPU unless given.
    ``reference``: a ``ScoreReference``; every complex must then be a pose of its table, and every molecule also gets
    ``score/irmsd``, ``score/lrmsd``, ``score/fnat``, ``score/dockQ``, ``score/binclass``, ``score/capri_class``.
    ``bsa``: True, or a ``radii`` value of ``residue_bsa`` ("reference", "protor", a pair of arrays): every molecule also
    gets ``node_data/bsa``, float64 [n,1], the buried surface area of exactly its nodes (one more launch per chunk).
    ``hse``: True, or a dict of ``residue_hse`` options (radius, offset, connect, direction): every molecule also gets
    ``node_data/hse``, float64 [n,3], the half-sphere exposure (up, down, angle) of exactly its nodes (one more launch
    per chunk); a node without a value has the row (0, 0, 0), as in the reference.
    ``depth``: True, or a dict of ``residue_depth`` options (radii, probe, n_dots, link, components): every molecule also
    gets ``node_data/depth``, float64 [n], the residue depth of exactly its nodes (three more launches per chunk).
    ``lddt``: an ``LddtReference``; every complex must then be a pose of its table, and every molecule also gets
    ``score/lddt``, ``score/ilddt`` and ``node_data/lddt``, float64 [n], the per-residue lDDT of exactly its nodes (0 for
    a residue without a reference pair)."""
    from .dataset import GraphStore
    api = api or _lib.get()
    device = _default_device(api, device)
    cx = _complexes(tables_or_poses)
    names = [str(n) for n in names]
    if len(names) != len(cx):
        raise ValueError("%d names for %d complexes" % (len(names), len(cx)))
    if reference is not None and not all(t is reference.table for t, _ in cx):
        raise ValueError("with `reference`, every complex must be a pose of the reference's AtomTable")
    if lddt is not None and not all(t is lddt.table for t, _ in cx):
        raise ValueError("with `lddt`, every complex must be a pose of the reference's AtomTable")
    active = [(f,) + f.options(value, [t for t, _ in cx])              # the options and the host tables refuse before any launch
              for f, value in zip(FEATURES, (bsa, hse, depth)) if value is not None and value is not False]
    if chunk is None:
        chunk = default_chunk(api, max([t.split for t, _ in cx] + [0]), max([t.n_residues - t.split for t, _ in cx] + [0]),
                              max([t.n_atoms for t, _ in cx] + [0]))
    chunk = max(1, int(chunk))
    trees = []
    for lo in range(0, len(cx), chunk):
        part = cx[lo:lo + chunk]
        ragged = _ragged(part)
        res_ptr = ragged[2]
        r = build_ragged(api, *ragged, contact_distance, internal_contact_distance, device)
        node_res = [r["node_residue"][r["node_ptr"][k]:r["node_ptr"][k + 1]].astype(np.int64) - int(res_ptr[k])
                    for k in range(len(part))]
        rows = [_feature_chunk(f, api, part, node_res, tabs_of, opt, device, ragged=ragged) for f, opt, tabs_of in active]
        for k, (t, _) in enumerate(part):
            n0, n1 = r["node_ptr"][k:k + 2]
            e0, e1 = r["edge_ptr"][k:k + 2]
            i0, i1 = r["iedge_ptr"][k:k + 2]
            residue = node_res[k]
            typ = r["type"][n0:n1].astype(np.int64)
            trees.append({
                "nodes": np.stack((np.asarray(t.chains)[t.res_chain[residue]], t.res_seq[residue].astype("U"),
                                   t.res_name[residue]), axis=1).astype("S") if n1 > n0 else np.zeros((0, 3), "S1"),
                "edge_index": r["edge_index"][e0:e1].copy(),
                "edge_data/dist": r["dist"][e0:e1].copy(),
                "internal_edge_index": r["internal_edge_index"][i0:i1].copy(),
                "internal_edge_data/dist": r["internal_dist"][i0:i1].copy(),
                "node_data/pos": r["pos"][n0:n1].copy(),
                "node_data/chain": r["chain"][n0:n1].astype(np.int64),
                "node_data/type": np.eye(20, dtype=np.float32)[typ],
                "node_data/polarity": np.eye(4, dtype=np.float32)[RESIDUE_POLARITY[typ]],
                "node_data/charge": RESIDUE_CHARGE[typ].astype(np.float64),
                "node_data/residue": residue,
            })
            for (f, _, _), per_complex in zip(active, rows):
                trees[-1]["node_data/" + f.name] = f.node_data(per_complex[k])
    store = GraphStore.from_trees(names, trees)
    if reference is not None and cx:
        attach_scores(store, names, docking_scores(np.stack([x for _, x in cx]), reference, device=device, api=api))
    if lddt is not None and cx:
        scores = lddt_scores(np.stack([x for _, x in cx]), lddt, per_residue=True, device=device, api=api)
        attach_scores(store, names, scores)
        for m, mol in enumerate(names):
            per_residue = scores["residue_lddt"][m]
            store.set(mol, "node_data/lddt", np.where(np.isnan(per_residue), 0.0, per_residue)[store.get(mol, "node_data/residue")])
    return store


def attach_residue_features(store, name, per_residue_array):
    """``node_data/<name>`` of every molecule of ``store`` = ``per_residue_array[node_data/residue]``: a table with
    one row per residue of the ``AtomTable`` (pssm, ic, cons ... constant across rigid-body poses), or a dict
    ``{mol: table}``."""
    for mol in store.mols():
        table = per_residue_array[mol] if isinstance(per_residue_array, dict) else per_residue_array
        store.set(mol, "node_data/" + name, np.asarray(table)[store.get(mol, "node_data/residue")])
    return store


# ---- resident graph sets without host trees (csrc/drgnn_pack.h) --------------------------------------------------------
# the (source, column) pairs of drgnn_iface_pack behind every built-in node feature
PACK_SOURCE = dict({"type": [(_lib.PACK_TYPE, j) for j in range(20)], "polarity": [(_lib.PACK_TYPE, 20 + j) for j in range(4)],
                    "charge": [(_lib.PACK_TYPE, 24)], "pos": [(_lib.PACK_POS, j) for j in range(3)], "chain": [(_lib.PACK_CHAIN, 0)]},
                   **{f.name: f.pack for f in FEATURES})               # bsa, hse, depth
FEATURE_WIDTH = {name: len(cols) for name, cols in PACK_SOURCE.items()}    # columns of x behind every built-in node feature
MCL_WORKSPACE_BUDGET = 256 << 20   # bytes of Markov clustering's dense fp64 workspace (3 n^2 per graph) one precluster call may ask for


def pack_type_table():
    """float32 [20, 25]: row = residue type; columns 0 - 19 the one-hot ``type``, 20 - 23 the one-hot ``polarity``, 24
    the ``charge``: the rows ``interface_graphs`` writes per node, rounded to float32 as the store path rounds them."""
    t = np.zeros((20, 25), dtype=np.float32)
    t[:, :20] = np.eye(20, dtype=np.float32)
    t[np.arange(20), 20 + RESIDUE_POLARITY] = 1.0
    t[:, 24] = RESIDUE_CHARGE.astype(np.float32)
    return t


def _pack_columns(node_feature, residue_width):
    """cols int32 [F,2] of drgnn_iface_pack for the feature names in order; residue_width: {name: (offset, width)}"""
    cols = []
    for name in node_feature:
        if name in PACK_SOURCE:
            cols += PACK_SOURCE[name]
        else:
            off, w = residue_width[name]
            cols += [(_lib.PACK_RES, off + j) for j in range(w)]
    return np.ascontiguousarray(np.array(cols, dtype=np.int32).reshape(-1, 2))


def iface_pack_raw(api, built, ptrs, cols, n_residues, type_table=None, bsa=None, hse=None, res_feat=None, edge_mode=1,
                   want=("x", "edge_index", "edge_attr", "internal_edge_index", "batch"), depth=None):
    """One drgnn_iface_pack call (include/drgnn.h) over what ``build_ragged_device`` returned (``built``, ``ptrs``), all
    on the device: a dict of the outputs named in ``want``.  ``cols`` int32 [F,2] on the host; ``type_table`` / ``bsa`` /
    ``hse`` / ``res_feat`` / ``depth``: device tensors (float32 [20,Wt], float64 [N,3], float64 [N,3], float32 [n_rows,W],
    float64 [N])."""
    r, out = _pack_fill(built, ptrs, cols, n_residues, type_table, bsa, hse, res_feat, edge_mode, want, depth)
    r.run(api, "iface_pack")
    return out


def pack_request(built, ptrs, cols, n_residues, type_table=None, bsa=None, hse=None, res_feat=None, edge_mode=1,
                 want=("x", "edge_index", "edge_attr", "internal_edge_index", "batch"), depth=None):
    """(drgnn_pack_request, its freshly allocated outputs, the arrays the request points into) of ``iface_pack_raw``"""
    r, out = _pack_fill(built, ptrs, cols, n_residues, type_table, bsa, hse, res_feat, edge_mode, want, depth)
    return r.q, out, tuple(r.held)


def _pack_fill(built, ptrs, cols, n_residues, type_table, bsa, hse, res_feat, edge_mode, want, depth):
    """(the filled Request, its outputs by name) of ``pack_request``"""
    M = int(ptrs.shape[1]) - 1
    N, E, Ei = int(built["pos"].shape[0]), int(built["dist"].shape[0]), int(built["internal_edge_index"].shape[0])
    for name, rows, shape in (("bsa", bsa, (N, 3)), ("hse", hse, (N, 3)), ("depth", depth, (N,))):    # (the kernel reads row i of node i)
        if rows is not None and (tuple(rows.shape) != shape or rows.dtype != torch.float64 or not rows.is_contiguous()):
            raise ValueError("%s must be float64 %s, one row per node" % (name, list(shape)))
    for name, t, dt in (("type_table", type_table, torch.float32), ("res_feat", res_feat, torch.float32)):
        if t is not None and (t.dim() != 2 or t.dtype != dt or not t.is_contiguous() or (name == "type_table" and t.shape[0] != 20)):
            raise ValueError("%s must be a contiguous float32 matrix%s" % (name, " of 20 rows" if name == "type_table" else ""))
    r = Request(_lib.PackRequest, ptrs.device)
    F = int(r.table("cols", cols, shape=(-1, 2))[0].shape[0])
    for name, row in zip(("node_ptr", "edge_ptr", "iedge_ptr"), ptrs):
        r.input(name, row)
    for name in ("node_residue", "chain", "type", "pos", "edge_index", "dist", "internal_edge_index"):
        r.input(name, built[name])
    for name, t in (("bsa", bsa), ("hse", hse), ("depth", depth), ("res_feat", res_feat), ("type_table", type_table)):
        r.input(name, t)
    r.set(n_complexes=M, n_nodes=N, n_edges=E, n_iedges=Ei, n_residues=int(n_residues), n_cols=F, edge_mode=int(edge_mode),
          n_rows=0 if res_feat is None else int(res_feat.shape[0]), res_width=0 if res_feat is None else int(res_feat.shape[1]),
          type_width=0 if type_table is None else int(type_table.shape[1]))
    shapes = {"x": ("x", (N, F), torch.float32), "edge_index": ("edge_index_out", (2, 2 * E), torch.int64),
              "edge_attr": ("edge_attr", 2 * E, torch.float32),
              "internal_edge_index": ("internal_edge_index_out", (2, 2 * Ei), torch.int64), "batch": ("batch", N, torch.int64)}
    return r, {name: r.output(*shapes[name]) for name in shapes if name in want}


def _residue_tables(residue_features, cx, names):
    """{feature: (offset, width)}, the total width, and rows(k) -> float32 [R_k, W] of complex k, after checking every
    table against its AtomTable: a wrongly shaped one raises ValueError"""
    widths, off = {}, 0
    per_complex = {}
    for feat, tab in (residue_features or {}).items():
        w = None
        for k, (t, _) in enumerate(cx):
            if isinstance(tab, dict) and names[k] not in tab:
                raise ValueError("residue feature %r has no table for %r" % (feat, names[k]))
            shape = np.shape(tab[names[k]] if isinstance(tab, dict) else tab)
            if len(shape) not in (1, 2) or shape[0] != t.n_residues or (len(shape) == 2 and shape[1] < 1):
                raise ValueError("residue feature %r of %r needs one row per residue (%d), got shape %r"
                                 % (feat, names[k], t.n_residues, shape))
            wk = 1 if len(shape) == 1 else int(shape[1])
            if w is not None and wk != w:
                raise ValueError("residue feature %r: %d columns for %r, %d before" % (feat, wk, names[k], w))
            w = wk
        w = w or 1                                                      # (no complex at all: any width does)
        widths[feat] = (off, w)
        per_complex[feat] = tab
        off += w
    made = {}

    def rows(k):
        """float32 [R_k, W]; the same object for complexes that share every table"""
        key = tuple(id(tab[names[k]]) if isinstance(tab, dict) else id(tab) for tab in per_complex.values())
        if key not in made:
            parts = [np.asarray(tab[names[k]] if isinstance(tab, dict) else tab, dtype=np.float64).reshape(cx[k][0].n_residues, -1)
                     for tab in per_complex.values()]
            made[key] = np.ascontiguousarray(np.hstack(parts).astype(np.float32))
        return made[key]
    return widths, off, rows


def _mcl_groups(sizes, budget):
    """consecutive runs [lo, hi) of graphs whose 24 * sum n^2 bytes stay within ``budget`` (a graph beyond it alone)"""
    groups, lo, used = [], 0, 0
    for k, n in enumerate(sizes):
        need = 24 * int(n) * int(n)
        if k > lo and used + need > budget:
            groups.append((lo, k))
            lo, used = k, 0
        used += need
    if lo < len(sizes):
        groups.append((lo, len(sizes)))
    return groups


def interface_resident_set(tables_or_poses, names, node_feature=("type", "polarity", "bsa", "hse"), edge_feature=("dist",),
                           edge_transform="default", residue_features=None, reference=None, target=None,
                           clustering_method="mcl", bsa=True, hse=True, depth=None, contact_distance=8.5, internal_contact_distance=3.0,
                           chunk=None, device=None, api=None, mcl_budget=MCL_WORKSPACE_BUDGET):
    """The ``ResidentGraphSet`` of the interface graphs of complexes (as ``interface_graphs`` takes them), assembled on
    the device: what ``interface_graphs`` -> ``attach_residue_features`` -> ``GraphDataSet(node_feature, edge_feature,
    target, clustering_method)`` -> ``PreCluster`` -> ``ResidentGraphSet`` gives, bit for bit (``edge_attr`` with the
    default transform: within 2^-21, see below), without a host tree, a per-graph tensor or a second upload.

    ``node_feature``: names in the order of the columns of ``x``: ``type`` (20 columns), ``polarity`` (4), ``charge``,
    ``pos`` (3), ``chain``, ``bsa``, ``hse`` (3), ``depth`` and the keys of ``residue_features`` ({name: table with one row per
    residue of the AtomTable, or {mol: table}}, as ``attach_residue_features`` takes them).  ``"all"``, an unknown
    name or a wrongly shaped table raises ValueError before any launch.  ``bsa`` / ``hse`` / ``depth``: the options
    of ``interface_graphs``; they are computed only when a feature asks for them, and ``depth`` is a feature only when
    the argument is given (True or a dict).  All three reach ``x`` through the pack launch, rounded once to float32 as
    the store path rounds them; a feature listed twice gives two equal columns.
    ``edge_feature``: ``("dist",)`` or None (no ``edge_attr``).  ``edge_transform``: "default" (the reference's
    ``tanh(-d/2 + 2) + 1``, evaluated in fp64 on the float32 distance and rounded once, where the store path evaluates
    it in float32: the two differ by at most 2^-21), None (the distances as they are) or a callable applied to the
    device tensor of the distances [2E].
    ``reference`` and ``target``: ``y`` = ``docking_scores(...)[target]`` as float32, the value the store path reads
    from ``score/<target>``.  ``clustering_method``: 'mcl' or 'louvain'.

    A complex without a single node gets no graph (a net cannot score one): ``rs.mols`` are the kept names, in order,
    ``rs.skipped`` the others.

    Per ``chunk`` of complexes (default as for ``interface_graphs``): count and fill (``build_ragged_device``),
    ``bsa`` / ``hse`` / ``depth`` of exactly the nodes, one ``drgnn_iface_pack`` launch, ``precluster`` over runs of graphs whose
    dense Markov-clustering workspace (24 sum n^2 bytes) stays within ``mcl_budget``; after the last chunk one
    ``torch.cat`` per array.  What comes back to the host: the three totals of a chunk, its [M+1] offset tables, the
    offsets of the depth-0 clusters, the status words of the bsa / hse / depth calls and, when one of them is asked for,
    ``node_residue`` (their target lists are made on the host); nothing else.  The result does not depend on ``chunk``,
    on ``mcl_budget`` or on the run."""
    from .clustering import _labeller, precluster
    from .resident import ResidentGraphSet
    import types
    api = api or _lib.get()
    device = _default_device(api, device)
    cx = _complexes(tables_or_poses)
    names = [str(n) for n in names]
    if len(names) != len(cx):
        raise ValueError("%d names for %d complexes" % (len(names), len(cx)))
    if len(set(names)) != len(names):
        raise ValueError("the names must be unique")
    # ---- everything that can be refused, before any launch
    if isinstance(node_feature, str) or not len(node_feature):
        raise ValueError("node_feature must list the features by name (%s and the keys of residue_features), not %r"
                         % (", ".join(FEATURE_WIDTH), node_feature))
    node_feature = [str(f) for f in node_feature]
    residue_features = dict(residue_features or {})
    for f in residue_features:
        if f in FEATURE_WIDTH:
            raise ValueError("residue feature %r has the name of a built-in feature" % f)
    for f in node_feature:
        if f not in FEATURE_WIDTH and f not in residue_features:
            raise ValueError("unknown node feature %r: %s and the keys of residue_features" % (f, ", ".join(FEATURE_WIDTH)))
        if f == "depth" and (depth is None or depth is False):         # (built only on request: depth=True or its options)
            raise ValueError("unknown node feature 'depth' unless depth=True or a dict of residue_depth's options is given")
    if edge_feature is not None and list(edge_feature) != ["dist"]:
        raise ValueError("edge_feature must be ('dist',) or None, not %r" % (edge_feature,))
    if not (edge_transform is None or edge_transform == "default" or callable(edge_transform)):
        raise ValueError("edge_transform must be 'default', None or a callable, not %r" % (edge_transform,))
    _labeller(clustering_method)
    if (reference is None) != (target is None):
        raise ValueError("`reference` and `target` go together")
    if reference is not None:
        if target not in SCORE_KEYS:
            raise ValueError("target must be one of %s, not %r" % (", ".join(SCORE_KEYS), target))
        if not all(t is reference.table for t, _ in cx):
            raise ValueError("with `reference`, every complex must be a pose of the reference's AtomTable")
    used = {f: residue_features[f] for f in node_feature if f in residue_features}
    res_cols, res_width, res_rows = _residue_tables(used, cx, names)
    active = []
    for f, value in zip(FEATURES, (bsa, hse, depth)):
        if f.name in node_feature:
            if value is False or value is None:
                raise ValueError("the node feature %r needs %s=True or %s" % (f.name, f.name, f.needs))
            active.append((f,) + f.options(value, [t for t, _ in cx]))
    cols = _pack_columns(node_feature, res_cols)
    if cols.shape[0] > api.pack_capacity(0):
        raise ValueError("%d columns of node features; drgnn_iface_pack takes %d" % (cols.shape[0], api.pack_capacity(0)))
    if chunk is None:
        chunk = default_chunk(api, max([t.split for t, _ in cx] + [0]), max([t.n_residues - t.split for t, _ in cx] + [0]),
                              max([t.n_atoms for t, _ in cx] + [0]))
    chunk = max(1, min(int(chunk), api.pack_capacity(2)))
    # ---- the chunks
    rs = ResidentGraphSet.__new__(ResidentGraphSet)
    rs._open(device, api)
    dev = rs.device
    type_table = torch.from_numpy(pack_type_table()).to(dev)
    res_dev = {}                                                       # residue tables on the device, by identity
    edge_mode = 1 if (edge_feature is not None and edge_transform == "default") else 0
    want = ("x", "edge_index", "internal_edge_index", "batch") + (("edge_attr",) if edge_feature is not None else ())
    kept, skipped, parts = [], [], []
    n_nodes, n_edges, n_c1 = [], [], []
    for lo in range(0, len(cx), chunk):
        part = cx[lo:lo + chunk]
        M = len(part)
        ragged = _ragged(part)
        atom_ptr, res_ptr = ragged[1:3]
        built, ptrs = build_ragged_device(api, *ragged, contact_distance, internal_contact_distance, dev)
        hp = ptrs.cpu().numpy().astype(np.int64)                       # the [M+1] tables
        nn = np.diff(hp[0])
        for k in range(M):
            (kept if nn[k] > 0 else skipped).append(names[lo + k])
        if hp[0, -1] == 0:
            continue
        rows = {}                                                      # the rows of exactly the nodes, by feature, on the device
        if active:
            node_residue = built["node_residue"].cpu().numpy().astype(np.int64)
            node_res = [node_residue[hp[0, k]:hp[0, k + 1]] - int(res_ptr[k]) for k in range(M)]
            for f, opt, tabs_of in active:
                rows[f.name] = _feature_chunk(f, api, part, node_res, tabs_of, opt, dev, ragged=ragged, keep_device=True)
        d_res = None
        if res_width:
            tabs = [res_rows(lo + k) for k in range(M)]
            shared = all(t is tabs[0] for t in tabs) and all(t is part[0][0] for t, _ in part)
            key = id(tabs[0]) if shared else None
            if key is not None and key in res_dev:
                d_res = res_dev[key]
            else:
                d_res = torch.from_numpy(tabs[0] if shared else np.concatenate(tabs)).to(dev)
                if key is not None:
                    res_dev[key] = d_res
        out = iface_pack_raw(api, built, ptrs, cols, len(atom_ptr) - 1, type_table, res_feat=d_res, edge_mode=edge_mode,
                             want=want, **rows)
        if edge_feature is not None and callable(edge_transform):
            out["edge_attr"] = torch.as_tensor(edge_transform(out["edge_attr"]), device=dev).to(torch.float32).reshape(-1)
        # ---- clusters: the kept graphs of the chunk in runs that fit the budget
        live = np.flatnonzero(nn > 0)
        rank = np.full(M, -1, dtype=np.int64)
        rank[live] = np.arange(live.size)
        d_rank = torch.from_numpy(rank).to(dev)
        c0s, c1s = [], []
        for g0, g1 in _mcl_groups(nn[live], int(mcl_budget)):
            a, b = int(live[g0]), int(live[g1 - 1]) + 1                # complexes [a, b): the empty ones among them hold nothing
            na, nb, ia, ib = int(hp[0, a]), int(hp[0, b]), 2 * int(hp[2, a]), 2 * int(hp[2, b])
            shadow = types.SimpleNamespace(internal_edge_index=out["internal_edge_index"][:, ia:ib] - na,
                                           batch=d_rank[out["batch"][na:nb]] - g0, num_graphs=g1 - g0)
            d0, d1, cptr = precluster(shadow, method=clustering_method, api=api, with_cluster_ptr=True)
            c0s.append(d0)
            c1s.append(d1)
            n_c1 += np.diff(cptr.cpu().numpy().astype(np.int64)).tolist()       # the cluster-count table
        n_nodes += nn[live].tolist()
        n_edges += (2 * np.diff(hp[1])[live]).tolist()
        out["cluster0"], out["cluster1"] = torch.cat(c0s), torch.cat(c1s)
        parts.append(out)

    def cat(key, dim=0, empty=None):
        return torch.cat([p[key] for p in parts], dim=dim) if parts else empty
    y = None
    if reference is not None:
        scores = docking_scores(np.stack([x for _, x in cx]), reference, device=dev, api=api) if cx else {target: np.zeros(0)}
        keep = np.array([n not in set(skipped) for n in names], dtype=bool)
        y = torch.from_numpy(np.asarray(scores[target])[keep].astype(np.float32))       # (host: _adopt keeps it as y_host)
    F = int(cols.shape[0])
    rs._adopt(mols=kept, n_nodes=n_nodes, n_edges=n_edges, n_c1=n_c1,
              x=cat("x", empty=torch.zeros((0, F), dtype=torch.float32, device=dev)),
              edge_index=cat("edge_index", dim=1, empty=torch.zeros((2, 0), dtype=torch.int64, device=dev)),
              edge_attr=None if edge_feature is None else cat("edge_attr", empty=torch.zeros(0, dtype=torch.float32, device=dev)),
              cluster0=cat("cluster0", empty=torch.zeros(0, dtype=torch.int64, device=dev)),
              cluster1=cat("cluster1", empty=torch.zeros(0, dtype=torch.int64, device=dev)), y=y)
    rs.skipped = skipped
    return rs
