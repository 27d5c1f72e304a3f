"""Interface graphs from atom coordinates, built on the device: the geometric half of the reference's graph
generation (``ResidueGraph`` / ``GraphGenMP``: ResidueGraph.py:108-145, 207-245, 272-316, 364-381).

    chain, res_seq, res_name, xyz = read_pdb_atoms("1ATN_1w.pdb")
    table = AtomTable(chain, res_seq, res_name, xyz)
    store = interface_graphs([table], ["1ATN_1w"])           # a GraphStore: GraphDataSet / PreCluster / NeuralNet take it

    poses = AtomTable.poses(table, xyz_of_all_poses)         # docking: one topology, M coordinate sets
    store = interface_graphs(poses, names)

Covered: nodes, interface and internal edges with their ``dist``, and the node features that come from the
coordinates or from a table (``pos``, ``chain``, ``type``, ``polarity``, ``charge``), and the scores against a
reference structure (``irmsd``, ``lrmsd``, ``fnat``, ``dockQ``, ``binclass``, ``capri_class``: Graph.get_score,
Graph.py:27-59):

    names = read_pdb_atom_names("1ATN_1w.pdb")
    table = AtomTable(chain, res_seq, res_name, xyz, atom_name=names)
    rc, rs, _, rx = read_pdb_atoms("1ATN.pdb"); rn = read_pdb_atom_names("1ATN.pdb")
    ref = ScoreReference(table, rc, rs, rn, rx)                # once per complex, on the host
    scores = docking_scores(poses, ref)                        # dict of arrays [M], one launch per chunk of poses
    store = interface_graphs(poses, names, reference=ref)      # the graphs with score/<target> on every molecule

and the buried surface area of the interface residues (``bsa``: tools/BSA.py through freesasa's Lee-Richards
method, with the reference's radii), which needs the atom names:

    areas = residue_bsa(poses)                                 # float64 [M, R]: every residue of every pose
    store = interface_graphs(poses, names, bsa=True)           # the graphs with node_data/bsa on every molecule

and the half-sphere exposure of the residues (``hse``: Biopython's HSExposureCA, radius 12 A, as up, down, angle),
which needs the atom names too:

    exposure = residue_hse(poses)                              # float64 [M, R, 3]; NaN rows: residues without a value
    store = interface_graphs(poses, names, hse=True)           # the graphs with node_data/hse on every molecule

``AtomTable`` keeps two chains and merges insertion codes into their residue number, so ``hse`` equals the
reference's on two-chain complexes without insertion codes.

To score or train on the poses without going through a store, ``interface_resident_set`` packs the same graphs on the
device (csrc/drgnn_pack.h) into the ``ResidentGraphSet`` that ``NeuralNet.test`` and ``Ensemble.predict`` take:

    rs = interface_resident_set(poses, names, node_feature=["type", "polarity", "bsa", "hse", "pssm"],
                                residue_features={"pssm": table_R_by_20}, reference=ref, target="irmsd")

After scoring, the poses are clustered by the fraction of common contacts of their interfaces (FCC, the rule of
HADDOCK's ``cluster_fcc``; csrc/drgnn_fcc.h) and the clusters ranked by their best members:

    clusters = cluster_poses(poses)                            # labels [M] (-1: in no cluster), centres, sizes
    order, means = clusters.rank(scores, top=4)                # scores [M]: Ensemble.predict or docking_scores()[key]

or by their pairwise RMSD (the rule of HADDOCK's ``cluster_struc`` and of ClusPro; csrc/drgnn_rmsd.h):

    D = pose_rmsd(poses, kind="ligand")                        # float64 [M, M] on the device: pairwise l-RMSD
    clusters = cluster_poses_rmsd(D, cutoff=7.5, min_size=4)   # the same PoseClusters

A set too large for the pairwise stages is first looked at as a whole (CONSRANK: how often the poses have each contact,
and how well each pose agrees with that; csrc/drgnn_consensus.h), linear in the poses:

    c = pose_contacts(all_decoys)                              # 10^4 - 10^5 poses
    best = np.argsort(-consensus_scores(c))[:4096]             # the poses that agree best with the set
    clusters = cluster_poses(c.select(best))
    maps = consensus_contacts(clusters.consensus(c.select(best)))   # a PoseContacts: the consensus contacts of every cluster

and the residue depth (``depth``: Biopython's residue depth; the surface is a dot surface of the solvent-accessible
surface restricted to its outer component instead of MSMS' triangulation, about one vertex spacing away from it):

    depth = residue_depth(poses)                               # float64 [M, R]
    store = interface_graphs(poses, names, depth=True)         # the graphs with node_data/depth on every molecule

Not covered: PSSM file parsing (``pssm``, ``cons``, ``ic``).  For those every
graph carries ``node_data/residue``, each node's index among the residues of its
``AtomTable``: a per-residue array the caller holds is attached with ``attach_residue_features``.

Order (fixed here; the reference's is networkx insertion order): nodes by (chain, position of the residue in the
input), interface edges (A node, B node) and internal edges (i < j) sorted by their pair.
"""
import collections
import ctypes

import numpy as np
import torch

from . import _lib

# this reference version's tables (ResidueGraph.py:43-60): index = the `type` of the residue
RESIDUE_NAMES = ("CYS", "HIS", "ASN", "GLN", "SER", "THR", "TYR", "TRP", "ALA", "PHE",
                 "GLY", "ILE", "VAL", "MET", "PRO", "LEU", "GLU", "ASP", "LYS", "ARG")
RESIDUE_CHARGE = np.array([-0.64, -0.29, -1.22, -1.22, -0.80, -0.80, -0.80, -0.79, -0.37, -0.37,
                           -0.37, -0.37, -0.37, -0.37, 0.0, -0.37, -1.37, -1.37, -0.36, -1.65])
# 0 apolar, 1 polar, 2 negatively charged, 3 positively charged (LYS is listed as negatively charged there)
RESIDUE_POLARITY = np.array([1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0, 2, 2, 2, 3])
_TYPE_OF = {n: i for i, n in enumerate(RESIDUE_NAMES)}
WORKSPACE_BUDGET = 256 << 20       # bytes of dense min-d^2 workspace one call may ask for (sets the default chunk)


def _default_device(api, device):
    """``device`` as given; None: where ``api`` computes (the GPU for the product library, the host for any other)"""
    return device if device is not None else "cuda" if api is _lib._API else "cpu"


def read_pdb_atoms(path):
    """(chain str [T], res_seq int32 [T], res_name str [T], xyz float64 [T,3]) of the ``ATOM`` records of a PDB file,
    by the fixed columns of the format, hydrogens included, in file order.  Host-side plumbing."""
    chain, seq, name, xyz = [], [], [], []
    with open(path) as f:
        for line in f:
            if line.startswith("ATOM  "):
                name.append(line[17:20].strip())
                chain.append(line[21])
                seq.append(int(line[22:26]))
                xyz.append((float(line[30:38]), float(line[38:46]), float(line[46:54])))
    return (np.array(chain, dtype="U1"), np.array(seq, dtype=np.int32), np.array(name, dtype="U3"),
            np.array(xyz, dtype=np.float64).reshape(-1, 3))


def read_pdb_atom_names(path):
    """atom names str [T] (columns 13-16, stripped) of the ``ATOM`` records of a PDB file: the records and the order
    of ``read_pdb_atoms``."""
    names = []
    with open(path) as f:
        for line in f:
            if line.startswith("ATOM  "):
                names.append(line[12:16].strip())
    return np.array(names, dtype="U4")


class AtomTable(object):
    """The atoms of one two-chain complex grouped for the kernels: atoms sorted by residue, residues of chain A
    (in order of first appearance in the input) before those of chain B.  A residue is (chain, res_seq).

    ``order`` [T] input position of each kept atom; ``atom_ptr`` int32 [R+1]; ``split`` = number of chain-A residues;
    ``res_chain`` / ``res_seq`` / ``res_name`` / ``res_type`` per residue (type -1: not one of the 20 standard names);
    ``xyz`` float32 [T,3] in the grouped order; ``atom_name`` [T] in the grouped order when given (the scores match
    atoms by it), else None."""

    def __init__(self, chain, res_seq, res_name, xyz, chains=("A", "B"), atom_name=None):
        chain = np.asarray(chain).astype("U")
        res_seq = np.asarray(res_seq).astype(np.int64)
        res_name = np.asarray(res_name).astype("U")
        xyz = np.asarray(xyz)
        if not (chain.shape == res_seq.shape == res_name.shape == xyz.shape[:1]) or xyz.shape[1:] != (3,):
            raise ValueError("chain, res_seq, res_name [T] and xyz [T,3] must describe the same atoms")
        side = np.full(chain.shape, -1, dtype=np.int64)
        side[chain == chains[0]] = 0
        side[chain == chains[1]] = 1
        kept = np.flatnonzero(side >= 0)
        # residue of every kept atom: rank of (side, first appearance of its (side, res_seq))
        span = int(res_seq.max() - res_seq.min() + 1) if kept.size else 1
        key = side[kept] * span + (res_seq[kept] - (res_seq.min() if kept.size else 0))
        uniq, first, inv = np.unique(key, return_index=True, return_inverse=True)
        rank_of_uniq = np.empty(len(uniq), dtype=np.int64)
        rank_of_uniq[np.lexsort((first, uniq // span))] = np.arange(len(uniq))
        res_of_atom = rank_of_uniq[inv]
        grouped = np.argsort(res_of_atom, kind="stable")
        self.order = kept[grouped]
        counts = np.bincount(res_of_atom, minlength=len(uniq))
        self.atom_ptr = np.concatenate(([0], np.cumsum(counts))).astype(np.int32)
        head = self.order[self.atom_ptr[:-1]] if len(uniq) else np.zeros(0, dtype=np.int64)
        self.res_chain = side[head].astype(np.int32)
        self.res_seq = res_seq[head].astype(np.int32)
        self.res_name = res_name[head]
        self.res_type = np.array([_TYPE_OF.get(n, -1) for n in self.res_name], dtype=np.int32)
        self.split = int((self.res_chain == 0).sum())
        self.chains = tuple(chains)
        self.n_input_atoms = int(chain.shape[0])
        self.xyz = np.ascontiguousarray(xyz[self.order], dtype=np.float32)
        self.atom_name = None
        if atom_name is not None:
            atom_name = np.asarray(atom_name).astype("U")
            if atom_name.shape != chain.shape:
                raise ValueError("atom_name [T] must describe the same atoms")
            self.atom_name = atom_name[self.order]

    @property
    def n_residues(self):
        return int(self.res_type.shape[0])

    @property
    def n_atoms(self):
        return int(self.order.shape[0])

    @staticmethod
    def poses(table, xyz):
        """M coordinate sets xyz [M, T, 3] (atoms in the order the table was made from) of one topology: the
        grouping of ``table`` is applied to all of them with one gather."""
        return Poses(table, xyz)


class Poses(object):
    """``AtomTable.poses``: ``table`` and ``xyz`` float32 [M, T', 3] in the table's grouped atom order."""

    def __init__(self, table, xyz):
        xyz = np.asarray(xyz)
        if xyz.ndim != 3 or xyz.shape[1:] != (table.n_input_atoms, 3):
            raise ValueError("poses need xyz [M, %d, 3]" % table.n_input_atoms)
        self.table = table
        self.xyz = np.ascontiguousarray(xyz[:, table.order], dtype=np.float32)

    def __len__(self):
        return int(self.xyz.shape[0])


def _complexes(items):
    """[(table, xyz float32 [T,3])] of a Poses, an AtomTable or a sequence of either"""
    if isinstance(items, Poses):
        return [(items.table, items.xyz[m]) for m in range(len(items))]
    if isinstance(items, AtomTable):
        return [(items, items.xyz)]
    out = []
    for it in items:
        out += _complexes(it)
    return out


def _ragged(part):
    """(xyz, atom_ptr, res_ptr, res_split, res_type) of a list of (table, xyz); the offset tables int32"""
    tables = [t for t, _ in part]
    m = len(part)
    xyz = np.concatenate([x for _, x in part]).astype(np.float32, copy=False) if m else np.zeros((0, 3), np.float32)
    if m and all(t is tables[0] for t in tables):                      # poses of one topology: no per-complex work
        t = tables[0]
        atom_ptr = np.append((t.atom_ptr[None, :-1].astype(np.int64) + t.n_atoms * np.arange(m)[:, None]).ravel(), m * t.n_atoms)
        res_ptr = t.n_residues * np.arange(m + 1)
        res_type = np.tile(t.res_type, m)
        split = res_ptr[:-1] + t.split
    else:
        n_at = np.array([t.n_atoms for t in tables], dtype=np.int64)
        n_res = np.array([t.n_residues for t in tables], dtype=np.int64)
        a0 = np.concatenate(([0], np.cumsum(n_at)))
        res_ptr = np.concatenate(([0], np.cumsum(n_res)))
        atom_ptr = np.concatenate([t.atom_ptr[:-1].astype(np.int64) + a0[k] for k, t in enumerate(tables)] + [a0[-1:]])
        res_type = np.concatenate([t.res_type for t in tables]) if m else np.zeros(0, np.int32)
        split = res_ptr[:-1] + np.array([t.split for t in tables], dtype=np.int64)
    if xyz.shape[0] * 3 >= 2 ** 31:
        raise ValueError("a chunk of %d complexes holds too many atoms for int32 offsets; lower `chunk`" % m)
    return (np.ascontiguousarray(xyz), atom_ptr.astype(np.int32), np.asarray(res_ptr).astype(np.int32),
            np.asarray(split).astype(np.int32), res_type.astype(np.int32))


def build_ragged_device(api, xyz, atom_ptr, res_ptr, res_split, res_type, contact_distance=8.5, internal_contact_distance=3.0,
                        device="cpu", tile_atoms=0, workspace_bytes=None):
    """One drgnn_iface_count + drgnn_iface_fill over a ragged batch given as numpy arrays (include/drgnn.h), the results
    left on ``device``: (out, ptrs) with ``out`` the dict of the eight outputs of drgnn_iface_fill as tensors and
    ``ptrs`` int32 [3, M+1] = node_ptr / edge_ptr / iedge_ptr.  Only the three totals come back to the host."""
    dev = torch.device(device)
    M, R = len(res_ptr) - 1, len(atom_ptr) - 1
    host = [np.ascontiguousarray(a, dtype=np.int32) for a in (atom_ptr, res_ptr, res_split)]
    d_xyz = torch.from_numpy(np.ascontiguousarray(xyz, dtype=np.float32)).to(dev)
    d_ap, d_rp, d_rs = [torch.from_numpy(h).to(dev) for h in host]
    d_rt = torch.from_numpy(np.ascontiguousarray(res_type, dtype=np.int32)).to(dev)
    if api is _lib._API:
        _lib.require_device(d_xyz)
    if workspace_bytes is None:
        rp, rs = host[1].astype(np.int64), host[2].astype(np.int64)
        workspace_bytes = api.iface_workspace_bytes(M, int((rs - rp[:-1]).max()) if M else 0,
                                                    int((rp[1:] - rs).max()) if M else 0, R)
    ws = torch.empty(max(int(workspace_bytes), 16), dtype=torch.uint8, device=dev)
    ptrs = torch.zeros((3, M + 1), dtype=torch.int32, device=dev)
    q = _lib.IfaceRequest()
    q.xyz, q.atom_ptr, q.res_ptr, q.res_split, q.res_type = (d_xyz.data_ptr(), d_ap.data_ptr(), d_rp.data_ptr(),
                                                            d_rs.data_ptr(), d_rt.data_ptr())
    q.host_atom_ptr, q.host_res_ptr, q.host_res_split = [h.ctypes.data for h in host]
    q.n_atoms, q.n_residues, q.n_complexes = int(d_xyz.shape[0]), R, M
    q.contact_distance, q.internal_contact_distance = float(contact_distance), float(internal_contact_distance)
    q.tile_atoms = int(tile_atoms)
    q.workspace, q.workspace_bytes = ws.data_ptr(), int(workspace_bytes)
    q.node_ptr, q.edge_ptr, q.iedge_ptr = ptrs[0].data_ptr(), ptrs[1].data_ptr(), ptrs[2].data_ptr()
    stream = _lib.current_stream(d_xyz)
    api.iface_count(q, stream)
    N, E, Ei = (int(v) for v in ptrs[:, -1].cpu())                 # the one synchronisation of the build
    out = {"node_residue": torch.empty(N, dtype=torch.int32, device=dev), "pos": torch.empty((N, 3), dtype=torch.float32, device=dev),
           "chain": torch.empty(N, dtype=torch.int32, device=dev), "type": torch.empty(N, dtype=torch.int32, device=dev),
           "edge_index": torch.empty((E, 2), dtype=torch.int64, device=dev), "dist": torch.empty(E, dtype=torch.float32, device=dev),
           "internal_edge_index": torch.empty((Ei, 2), dtype=torch.int64, device=dev),
           "internal_dist": torch.empty(Ei, dtype=torch.float32, device=dev)}
    api.iface_fill(q, N, E, Ei, out["node_residue"], out["pos"], out["chain"], out["type"], out["edge_index"], out["dist"],
                   out["internal_edge_index"], out["internal_dist"], stream)
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
                     api=None, reference=None, bsa=False, hse=False, depth=False):
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
    gets ``node_data/depth``, float64 [n], the residue depth of exactly its nodes (three more launches per chunk)."""
    from .dataset import GraphStore
    api = api or _lib.get()
    device = _default_device(api, device)
    cx = _complexes(tables_or_poses)
    names = [str(n) for n in names]
    if len(names) != len(cx):
        raise ValueError("%d names for %d complexes" % (len(names), len(cx)))
    if reference is not None and not all(t is reference.table for t, _ in cx):
        raise ValueError("with `reference`, every complex must be a pose of the reference's AtomTable")
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
# the (source, column) pairs of drgnn_iface_pack behind every built-in node feature; FEATURES (below) adds bsa, hse, depth
PACK_SOURCE = {"type": [(_lib.PACK_TYPE, j) for j in range(20)], "polarity": [(_lib.PACK_TYPE, 20 + j) for j in range(4)],
               "charge": [(_lib.PACK_TYPE, 24)], "pos": [(_lib.PACK_POS, j) for j in range(3)], "chain": [(_lib.PACK_CHAIN, 0)]}
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
    q, out, _ = pack_request(built, ptrs, cols, n_residues, type_table, bsa, hse, res_feat, edge_mode, want, depth)
    api.iface_pack(q, _lib.current_stream(ptrs))
    return out


def pack_request(built, ptrs, cols, n_residues, type_table=None, bsa=None, hse=None, res_feat=None, edge_mode=1,
                 want=("x", "edge_index", "edge_attr", "internal_edge_index", "batch"), depth=None):
    """(drgnn_pack_request, its freshly allocated outputs, the arrays the request points into) of ``iface_pack_raw``"""
    dev = ptrs.device
    cols = np.ascontiguousarray(cols, dtype=np.int32).reshape(-1, 2)
    M = int(ptrs.shape[1]) - 1
    N, E, Ei = int(built["pos"].shape[0]), int(built["dist"].shape[0]), int(built["internal_edge_index"].shape[0])
    F = int(cols.shape[0])
    for name, rows, shape in (("bsa", bsa, (N, 3)), ("hse", hse, (N, 3)), ("depth", depth, (N,))):    # (the kernel reads row i of node i)
        if rows is not None and (tuple(rows.shape) != shape or rows.dtype != torch.float64 or not rows.is_contiguous()):
            raise ValueError("%s must be float64 %s, one row per node" % (name, list(shape)))
    for name, t, dt in (("type_table", type_table, torch.float32), ("res_feat", res_feat, torch.float32)):
        if t is not None and (t.dim() != 2 or t.dtype != dt or not t.is_contiguous() or (name == "type_table" and t.shape[0] != 20)):
            raise ValueError("%s must be a contiguous float32 matrix%s" % (name, " of 20 rows" if name == "type_table" else ""))
    d_cols = torch.from_numpy(cols).to(dev)
    out = {}
    if "x" in want:
        out["x"] = torch.empty((N, F), dtype=torch.float32, device=dev)
    if "edge_index" in want:
        out["edge_index"] = torch.empty((2, 2 * E), dtype=torch.int64, device=dev)
    if "edge_attr" in want:
        out["edge_attr"] = torch.empty(2 * E, dtype=torch.float32, device=dev)
    if "internal_edge_index" in want:
        out["internal_edge_index"] = torch.empty((2, 2 * Ei), dtype=torch.int64, device=dev)
    if "batch" in want:
        out["batch"] = torch.empty(N, dtype=torch.int64, device=dev)
    p = lambda t: None if t is None or t.numel() == 0 else t.data_ptr()
    q = _lib.PackRequest()
    q.node_ptr, q.edge_ptr, q.iedge_ptr = ptrs[0].data_ptr(), ptrs[1].data_ptr(), ptrs[2].data_ptr()
    q.node_residue, q.chain, q.type, q.pos = p(built["node_residue"]), p(built["chain"]), p(built["type"]), p(built["pos"])
    q.edge_index, q.dist, q.internal_edge_index = p(built["edge_index"]), p(built["dist"]), p(built["internal_edge_index"])
    q.bsa, q.hse, q.depth, q.res_feat, q.type_table = p(bsa), p(hse), p(depth), p(res_feat), p(type_table)
    q.cols, q.host_cols = p(d_cols), (cols.ctypes.data if F else None)
    q.n_complexes, q.n_nodes, q.n_edges, q.n_iedges, q.n_residues = M, N, E, Ei, int(n_residues)
    q.n_rows = 0 if res_feat is None else int(res_feat.shape[0])
    q.res_width = 0 if res_feat is None else int(res_feat.shape[1])
    q.type_width = 0 if type_table is None else int(type_table.shape[1])
    q.n_cols, q.edge_mode = F, int(edge_mode)
    q.x, q.edge_index_out, q.edge_attr = p(out.get("x")), p(out.get("edge_index")), p(out.get("edge_attr"))
    q.internal_edge_index_out, q.batch = p(out.get("internal_edge_index")), p(out.get("batch"))
    return q, out, (cols, d_cols)


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


# ---- docking scores (csrc/drgnn_score.h) -------------------------------------------------------------------------------
BACKBONE =("CA", "C", "N", "O")
SCORE_KEYS = ("irmsd", "lrmsd", "fnat", "dockQ", "binclass", "capri_class")
SCORE_XYZ_BUDGET = 256 << 20       # bytes of pose coordinates one call uploads (sets the default chunk)


def _residue_pairs(xyz_a, res_a, xyz_b, res_b, n_res_b, cutoff, rows=256):
    """sorted unique res_a * n_res_b + res_b over the atom pairs at d <= cutoff (float64), ``rows`` atoms of A at a
    time"""
    found = []
    for lo in range(0, xyz_a.shape[0], rows):
        d = xyz_a[lo:lo + rows, None, :] - xyz_b[None, :, :]
        i, j = np.nonzero(np.sqrt((d * d).sum(axis=2)) <= cutoff)
        found.append(np.unique(res_a[lo + i] * n_res_b + res_b[j]))
    return np.unique(np.concatenate(found)) if found else np.zeros(0, dtype=np.int64)


class ScoreReference(object):
    """The once-per-complex half of the scores, on the host: the reference structure's residue pairs (an atom pair at
    d <= ``fnat_cutoff``, all atoms) and interface zone (the residues of the pairs at d <= ``izone_cutoff``), the
    matching of the table's atoms to the reference's by (chain, res_seq, atom name), the long chain (more residues in
    the reference, the first chain on a tie) and the four tables ``drgnn_dock_scores`` takes (include/drgnn.h).

    ``ref_chain`` / ``ref_res_seq`` / ``ref_atom_name`` [N] and ``ref_xyz`` [N,3]: the reference's atoms in any order;
    it may hold other atoms, residues and numbering than the decoy: what does not match is ignored on both sides.
    ``n_ref_pairs``: the reference's residue pairs (fnat's denominator); ``n_pairs``: those whose two residues the
    decoy has; ``zone_sizes``: matched backbone atoms of (interface zone, long chain, short chain); ``long_chain``."""

    def __init__(self, table, ref_chain, ref_res_seq, ref_atom_name, ref_xyz, izone_cutoff=10.0, fnat_cutoff=5.0):
        if table.atom_name is None:
            raise ValueError("the scores match atoms by name: build the AtomTable with atom_name=")
        ref_chain = np.asarray(ref_chain).astype("U")
        seq = np.asarray(ref_res_seq).astype(np.int64)
        name = np.asarray(ref_atom_name).astype("U")
        xyz = np.asarray(ref_xyz, dtype=np.float64)
        if not (ref_chain.shape == seq.shape == name.shape == xyz.shape[:1]) or xyz.shape[1:] != (3,):
            raise ValueError("ref_chain, ref_res_seq, ref_atom_name [N] and ref_xyz [N,3] must describe the same atoms")
        self.table = table
        self.izone_cutoff, self.fnat_cutoff = float(izone_cutoff), float(fnat_cutoff)
        side = np.full(ref_chain.shape, -1, dtype=np.int64)
        side[ref_chain == table.chains[0]] = 0
        side[ref_chain == table.chains[1]] = 1
        at = [np.flatnonzero(side == s) for s in (0, 1)]
        useq, inv = zip(*[np.unique(seq[a], return_inverse=True) for a in at])       # residues of each chain by res_seq
        if len(useq[0]) == 0 or len(useq[1]) == 0:
            raise ValueError("the reference has no atoms of chain %r or %r" % tuple(table.chains))
        nb = len(useq[1])
        near = [_residue_pairs(xyz[at[0]], inv[0], xyz[at[1]], inv[1], nb, c) for c in (self.fnat_cutoff, self.izone_cutoff)]
        self.n_ref_pairs = int(near[0].shape[0])
        if self.n_ref_pairs == 0:
            raise ValueError("the reference has no residue pair within %g" % self.fnat_cutoff)
        zone = (set(useq[0][near[1] // nb].tolist()), set(useq[1][near[1] % nb].tolist()))
        self.long_chain = 0 if len(useq[0]) >= len(useq[1]) else 1
        # the table's residues by (side, res_seq); the reference pairs whose two residues the decoy has
        res_of = {(int(c), int(q)): r for r, (c, q) in enumerate(zip(table.res_chain, table.res_seq))}
        pairs = [(res_of.get((0, int(useq[0][k // nb]))), res_of.get((1, int(useq[1][k % nb])))) for k in near[0]]
        pairs = [p for p in pairs if p[0] is not None and p[1] is not None]
        self.pair_res = np.array(pairs, dtype=np.int32).reshape(-1, 2)
        # matching: the first reference atom of every (side, res_seq, name)
        ref_of = {}
        for k in np.flatnonzero(side >= 0)[::-1]:
            ref_of[(int(side[k]), int(seq[k]), str(name[k]))] = int(k)
        res_of_atom = np.repeat(np.arange(table.n_residues), np.diff(table.atom_ptr))
        zones = ([], [], [])
        for i in np.flatnonzero(np.isin(table.atom_name, BACKBONE)):
            r = res_of_atom[i]
            c, q = int(table.res_chain[r]), int(table.res_seq[r])
            k = ref_of.get((c, q, str(table.atom_name[i])))
            if k is None:
                continue
            if q in zone[c]:
                zones[0].append((i, k))
            zones[1 if c == self.long_chain else 2].append((i, k))
        self.zone_sizes = tuple(len(z) for z in zones)
        if min(self.zone_sizes) < 3:
            raise ValueError("a zone of fewer than 3 matched backbone atoms (interface, long chain, short chain: %d, %d, %d)"
                             % self.zone_sizes)
        both = np.array(zones[0] + zones[1] + zones[2], dtype=np.int64)
        self.zone_atom = np.ascontiguousarray(both[:, 0], dtype=np.int32)
        self.zone_ref = np.ascontiguousarray(xyz[both[:, 1]], dtype=np.float64)
        self.zone_ptr = np.concatenate(([0], np.cumsum(self.zone_sizes))).astype(np.int32)
        self.atom_ptr = np.ascontiguousarray(table.atom_ptr, dtype=np.int32)
        self._device = {}

    @property
    def n_pairs(self):
        return int(self.pair_res.shape[0])

    def device_tables(self, device):
        """(zone_atom, zone_ref, pair_res, atom_ptr) on ``device``, uploaded once"""
        key = str(torch.device(device))
        if key not in self._device:
            self._device[key] = tuple(torch.from_numpy(a).to(device) for a in
                                      (self.zone_atom, self.zone_ref, self.pair_res.reshape(-1), self.atom_ptr))
        return self._device[key]


def dock_scores_raw(api, xyz, zone_atom, zone_ptr, zone_ref, pair_res, atom_ptr, n_ref_pairs, fnat_cutoff=5.0, device="cpu",
                    tables=None):
    """One drgnn_dock_scores call (include/drgnn.h) over numpy arrays: xyz float32 [M,T,3].  Returns (scores float64
    [M,4], classes int32 [M,2], n_preserved int32 [M]) as numpy arrays.  ``tables``: the four index tables already on
    the device."""
    dev = torch.device(device)
    xyz = np.ascontiguousarray(xyz, dtype=np.float32)
    host = [np.ascontiguousarray(zone_atom, dtype=np.int32), np.ascontiguousarray(zone_ptr, dtype=np.int32),
            np.ascontiguousarray(np.asarray(pair_res).reshape(-1), dtype=np.int32), np.ascontiguousarray(atom_ptr, dtype=np.int32)]
    if host[1].shape != (4,) or xyz.ndim != 3 or xyz.shape[2] != 3:
        raise ValueError("zone_ptr [4] and xyz [M,T,3]")
    if tables is None:
        tables = (torch.from_numpy(host[0]).to(dev), torch.from_numpy(np.ascontiguousarray(zone_ref, dtype=np.float64)).to(dev),
                  torch.from_numpy(host[2]).to(dev), torch.from_numpy(host[3]).to(dev))
    d_xyz = torch.from_numpy(xyz).to(dev)
    if api is _lib._API:
        _lib.require_device(d_xyz)
    M = int(xyz.shape[0])
    scores = torch.empty((M, 4), dtype=torch.float64, device=dev)
    classes = torch.empty((M, 2), dtype=torch.int32, device=dev)
    kept = torch.empty(M, dtype=torch.int32, device=dev)
    q = _lib.ScoreRequest()
    q.xyz = d_xyz.data_ptr()
    q.zone_atom, q.zone_ref, q.pair_res, q.atom_ptr = [t.data_ptr() if t.numel() else None for t in tables]
    q.host_zone_atom, q.host_zone_ptr, q.host_pair_res, q.host_atom_ptr = [h.ctypes.data if h.size else None for h in host]
    q.n_poses, q.n_atoms, q.n_residues, q.n_pairs = M, int(xyz.shape[1]), len(host[3]) - 1, host[2].shape[0] // 2
    q.n_ref_pairs, q.fnat_cutoff = int(n_ref_pairs), float(fnat_cutoff)
    q.scores, q.classes, q.n_preserved = scores.data_ptr(), classes.data_ptr(), kept.data_ptr()
    api.dock_scores(q, _lib.current_stream(d_xyz))
    return scores.cpu().numpy(), classes.cpu().numpy(), kept.cpu().numpy()


def docking_scores(poses_or_table, reference, device=None, api=None, chunk=None):
    """The scores of M poses of ``reference.table`` (an ``AtomTable.poses`` batch, the table itself, or xyz float32
    [M,T,3] already in the table's grouped atom order) against ``reference``: a dict of numpy arrays [M], ``irmsd``,
    ``lrmsd`` (A), ``fnat``, ``dockQ`` float64, ``binclass``, ``capri_class``, ``n_preserved`` int64.  One launch per
    ``chunk`` poses (default: what keeps the uploaded coordinates within SCORE_XYZ_BUDGET bytes); a pose's result does
    not depend on the chunk, on its place in the batch or on the run."""
    api = api or _lib.get()
    device = _default_device(api, device)
    t, xyz = _pose_batch(poses_or_table, reference.table, "the poses must be of the reference's AtomTable")
    if chunk is None:
        chunk = SCORE_XYZ_BUDGET // (12 * max(t.n_atoms, 1))
    chunk = max(1, int(chunk))
    tables = reference.device_tables(device)
    parts = [dock_scores_raw(api, xyz[lo:lo + chunk], reference.zone_atom, reference.zone_ptr, reference.zone_ref,
                             reference.pair_res, reference.atom_ptr, reference.n_ref_pairs, reference.fnat_cutoff, device, tables)
             for lo in range(0, xyz.shape[0], chunk)]
    sc = np.concatenate([p[0] for p in parts]) if parts else np.zeros((0, 4))
    cl = np.concatenate([p[1] for p in parts]) if parts else np.zeros((0, 2), np.int32)
    kept = np.concatenate([p[2] for p in parts]) if parts else np.zeros(0, np.int32)
    return {"irmsd": sc[:, 0].copy(), "lrmsd": sc[:, 1].copy(), "fnat": sc[:, 2].copy(), "dockQ": sc[:, 3].copy(),
            "binclass": cl[:, 0].astype(np.int64), "capri_class": cl[:, 1].astype(np.int64), "n_preserved": kept.astype(np.int64)}


def attach_scores(store, names, scores):
    """``score/<key>`` of molecule ``names[i]`` of ``store`` = ``scores[key][i]`` for the keys of SCORE_KEYS that
    ``scores`` (what ``docking_scores`` returns) holds; ``binclass`` is stored as a bool, as the reference does."""
    for i, mol in enumerate(names):
        for k in SCORE_KEYS:
            if k in scores:
                v = scores[k][i]
                store.set(str(mol), "score/" + k, np.asarray(bool(v)) if k == "binclass" else np.asarray(v))
    return store


# ---- buried surface area (csrc/drgnn_bsa.h) ----------------------------------------------------------------------------
# ProtOr radii of the heavy atoms (the classifier freesasa applies to a PDB file): backbone, then the side chains
BSA_BACKBONE = {"N": 1.64, "CA": 1.88, "C": 1.61, "O": 1.42, "OXT": 1.46}
_C, _N, _O1, _O2, _S, _CT, _CR = 1.88, 1.64, 1.42, 1.46, 1.77, 1.61, 1.76          # _CT trigonal, _CR aromatic CH carbon
BSA_SIDE_CHAIN = {
    "ALA": {"CB": _C},
    "ARG": {"CB": _C, "CG": _C, "CD": _C, "NE": _N, "CZ": _CT, "NH1": _N, "NH2": _N},
    "ASN": {"CB": _C, "CG": _CT, "OD1": _O1, "ND2": _N},
    "ASP": {"CB": _C, "CG": _CT, "OD1": _O1, "OD2": _O2},
    "CYS": {"CB": _C, "SG": _S},
    "GLN": {"CB": _C, "CG": _C, "CD": _CT, "OE1": _O1, "NE2": _N},
    "GLU": {"CB": _C, "CG": _C, "CD": _CT, "OE1": _O1, "OE2": _O2},
    "GLY": {},
    "HIS": {"CB": _C, "CG": _CT, "ND1": _N, "CD2": _CR, "CE1": _CR, "NE2": _N},
    "ILE": {"CB": _C, "CG1": _C, "CG2": _C, "CD1": _C},
    "LEU": {"CB": _C, "CG": _C, "CD1": _C, "CD2": _C},
    "LYS": {"CB": _C, "CG": _C, "CD": _C, "CE": _C, "NZ": _N},
    "MET": {"CB": _C, "CG": _C, "SD": _S, "CE": _C},
    "PHE": {"CB": _C, "CG": _CT, "CD1": _CR, "CD2": _CR, "CE1": _CR, "CE2": _CR, "CZ": _CR},
    "PRO": {"CB": _C, "CG": _C, "CD": _C},
    "SER": {"CB": _C, "OG": _O2},
    "THR": {"CB": _C, "OG1": _O2, "CG2": _C},
    "TRP": {"CB": _C, "CG": _CT, "CD1": _CR, "CD2": _CT, "NE1": _N, "CE2": _CT, "CE3": _CR, "CZ2": _CR, "CZ3": _CR, "CH2": _CR},
    "TYR": {"CB": _C, "CG": _CT, "CD1": _CR, "CD2": _CR, "CE1": _CR, "CE2": _CR, "CZ": _CT, "OH": _O2},
    "VAL": {"CB": _C, "CG1": _C, "CG2": _C},
}
# the unbound chains of the reference: it hands freesasa only the first character of the atom name
BSA_FIRST_LETTER = {"C": 1.61, "N": 1.64, "O": 1.42, "S": 1.80, "H": 1.10}
RESIDUE_XYZ_BUDGET = 256 << 20     # bytes of coordinates one bsa / hse / depth call uploads (sets their default chunk)
BSA_XYZ_BUDGET = RESIDUE_XYZ_BUDGET                                    # (its first name)


def bsa_radii(table, radii="reference"):
    """(complex_r, unbound_r) float64 [T] in the table's grouped atom order; 0: the atom is absent from that state.

    "reference": what the reference's ``bsa`` feature uses.  Complex: heavy atoms only (the name does not start with
    H) with ProtOr radii by (residue, atom name); a heavy atom outside the table or a non-standard residue raises
    ValueError.  Unbound: every atom, hydrogens included, the radius from the first character of its name (C 1.61, N
    1.64, O 1.42, S 1.80, H 1.10; any other raises ValueError).  "protor": the complex radii for both states.
    A pair ``(complex_r, unbound_r)`` of arrays [n_input_atoms] in input atom order is taken as it is."""
    if isinstance(radii, str):
        if radii not in ("reference", "protor"):
            raise ValueError("radii must be 'reference', 'protor' or a pair of arrays, not %r" % radii)
        if table.atom_name is None:
            raise ValueError("the radius tables go by atom name: build the AtomTable with atom_name=")
        bad = np.flatnonzero(table.res_type < 0)
        if bad.size:
            r = int(bad[0])
            raise ValueError("no radii for the non-standard residue %s %s%d" % (table.res_name[r], table.chains[table.res_chain[r]],
                                                                               table.res_seq[r]))
        res_of_atom = np.repeat(np.arange(table.n_residues), np.diff(table.atom_ptr))
        cr = np.zeros(table.n_atoms)
        ur = np.zeros(table.n_atoms)
        for i, nm in enumerate(table.atom_name):
            nm = str(nm)
            if radii == "reference":
                if nm[:1] not in BSA_FIRST_LETTER:
                    raise ValueError("no radius for an atom whose name starts with %r (%s)" % (nm[:1], nm))
                ur[i] = BSA_FIRST_LETTER[nm[0]]
            if not nm.startswith("H"):
                res = str(table.res_name[res_of_atom[i]])
                rad = BSA_BACKBONE.get(nm, BSA_SIDE_CHAIN[res].get(nm))
                if rad is None:
                    raise ValueError("no ProtOr radius for the heavy atom %s of %s" % (nm, res))
                cr[i] = rad
        return (cr, cr.copy()) if radii == "protor" else (cr, ur)
    try:
        cr, ur = radii
    except (TypeError, ValueError):
        raise ValueError("radii must be 'reference', 'protor' or a pair (complex_r, unbound_r)")
    out = []
    for a in (cr, ur):
        a = np.asarray(a, dtype=np.float64)
        if a.shape != (table.n_input_atoms,):
            raise ValueError("radius arrays need %d entries, one per input atom" % table.n_input_atoms)
        if not np.all(a >= 0.0):                                       # (NaN fails too)
            raise ValueError("radii must be >= 0 (0: the atom is absent)")
        out.append(a[table.order])
    return tuple(out)


def bsa_raw(api, xyz, atom_ptr, res_ptr, res_split, rad_complex, rad_unbound, target_res, target_complex, probe=1.4,
            n_slices=20, device="cpu", keep_device=False):
    """One drgnn_bsa_residues call (include/drgnn.h) over numpy arrays.  Returns (out float64 [K,3]: sasa_unbound,
    sasa_complex, bsa; status int): bit 0 of status says a list overflowed (those residues are NaN).  ``keep_device``:
    ``out`` stays a tensor on ``device``; only the status word comes back."""
    dev = torch.device(device)
    host = [np.ascontiguousarray(a, dtype=np.int32) for a in (atom_ptr, res_ptr, res_split, target_res, target_complex)]
    rad = [np.ascontiguousarray(a, dtype=np.float32) for a in (rad_complex, rad_unbound)]
    if rad[0].shape != rad[1].shape or rad[0].ndim != 1 or host[3].shape != host[4].shape:
        raise ValueError("the two radius arrays, and the two target arrays, must have one length each")
    d_xyz = torch.from_numpy(np.ascontiguousarray(xyz, dtype=np.float32).reshape(-1, 3)).to(dev)
    if api is _lib._API:
        _lib.require_device(d_xyz)
    d_host = [torch.from_numpy(h).to(dev) for h in host]
    d_rad = [torch.from_numpy(a).to(dev) for a in rad]
    K = int(host[3].shape[0])
    out = torch.empty((K, 3), dtype=torch.float64, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    q = _lib.BsaRequest()
    q.xyz = d_xyz.data_ptr()
    q.atom_ptr, q.res_ptr, q.res_split, q.target_res, q.target_complex = [t.data_ptr() for t in d_host]
    q.rad_complex, q.rad_unbound = [t.data_ptr() for t in d_rad]
    (q.host_atom_ptr, q.host_res_ptr, q.host_res_split, q.host_target_res,
     q.host_target_complex) = [h.ctypes.data for h in host]
    q.n_atoms, q.n_residues, q.n_complexes = int(d_xyz.shape[0]), len(host[0]) - 1, len(host[1]) - 1
    q.n_targets, q.n_radii = K, int(rad[0].shape[0])
    q.probe, q.n_slices = float(probe), int(n_slices)
    q.out, q.status = out.data_ptr(), status.data_ptr()
    api.bsa_residues(q, _lib.current_stream(d_xyz))
    return (out if keep_device else out.cpu().numpy()), int(status.cpu()[0])


def _bsa_options(probe=1.4, n_slices=20):
    if int(n_slices) < 1:
        raise ValueError("n_slices must be at least 1")
    if not float(probe) >= 0.0:
        raise ValueError("probe must be >= 0")
    return {"probe": probe, "n_slices": n_slices}


def residue_bsa(tables_or_poses, residues=None, radii="reference", probe=1.4, n_slices=20, device=None, chunk=None, api=None,
                parts=False):
    """Buried surface area (A^2) of residues, on the device: SASA of the residue in its chain alone minus its SASA in
    the complex, each by the Lee-Richards slice method (``probe`` 1.4 A, ``n_slices`` 20: what the reference's ``bsa``
    node feature records, negative values included; see ``bsa_radii`` for ``radii``).

    An ``AtomTable`` gives float64 [R], an ``AtomTable.poses`` batch [M, R], a sequence of either a list of [R_k], with
    NaN for the residues not asked for.  ``residues``: None (all), an index array applied to every complex, or one
    index array per complex.  Only the atoms of the residues asked for are evaluated.  ``chunk``: complexes per
    launch; a residue's bits do not depend on it, on the batch or on ``residues``.  ``parts``: return (bsa,
    sasa_unbound, sasa_complex) instead.  More than 256 neighbours of one atom is refused (DrgnnError, capacity)."""
    rows = _residue_values(BSA, tables_or_poses, residues, radii, {"probe": probe, "n_slices": n_slices}, device, chunk, api)

    def pick(a):                                                       # the columns of a row: sasa_unbound, sasa_complex, bsa
        got = tuple(np.ascontiguousarray(a[..., j]) for j in ((2, 0, 1) if parts else (2,)))
        return got if parts else got[0]
    return [pick(a) for a in rows] if isinstance(rows, list) else pick(rows)


# ---- half-sphere exposure (csrc/drgnn_hse.h) ---------------------------------------------------------------------------
HSE_CONNECT = {"CA": (1, 1, 4.3), "CN": (2, 0, 1.8)}      # (column of bb in r, column in r + 1, cutoff in A)
HSE_DIRECTION = {"CA": 0, "CB": 1}
HSE_BACKBONE = ("N", "CA", "C", "CB")                     # the columns of the bb table
HSE_TILE = (4, 64)                                        # targets per workgroup: the fewest and the most
HSE_WORKGROUPS = 512                                      # a call aims at this many workgroups (two per compute unit)


def hse_table(table):
    """bb int32 [R,5] of an ``AtomTable`` made with ``atom_name``: the offsets of the first atoms named N, CA, C, CB
    inside every residue (-1: absent) and flags: bit 0 one of the 20 standard residue names, bit 1 GLY, bit 2 the first
    residue of its chain."""
    if table.atom_name is None:
        raise ValueError("hse finds the backbone by atom name: build the AtomTable with atom_name=")
    R = table.n_residues
    bb = np.full((R, 5), -1, dtype=np.int32)
    res_of_atom = np.repeat(np.arange(R), np.diff(table.atom_ptr))
    inside = np.arange(table.n_atoms) - table.atom_ptr[:-1][res_of_atom]
    for col, name in enumerate(HSE_BACKBONE):
        hit = np.flatnonzero(table.atom_name == name)[::-1]                # reversed: the first atom of a name wins
        bb[res_of_atom[hit], col] = inside[hit]
    start = np.ones(R, dtype=bool)
    start[1:] = table.res_chain[1:] != table.res_chain[:-1]
    bb[:, 4] = (table.res_type >= 0) * 1 + (table.res_name == "GLY") * 2 + start * 4
    return bb


def hse_tile(n_targets):
    """targets per workgroup for a call of ``n_targets``: small calls spread over many workgroups (1 pose of 1ATN, all
    residues: 8.0 us at 4 against 32.1 us at 64), large ones stage a complex fewer times (1024 poses: 2.46 ms at 64 against
    3.57 ms at 4); profiles/hse_ab.txt.  It changes no bit of the result."""
    return max(HSE_TILE[0], min(HSE_TILE[1], int(n_targets) // HSE_WORKGROUPS))


def _hse_options(radius=12.0, offset=0, connect="CA", direction="CA"):
    if connect not in HSE_CONNECT:
        raise ValueError("connect must be 'CA' or 'CN', not %r" % (connect,))
    if direction not in HSE_DIRECTION:
        raise ValueError("direction must be 'CA' or 'CB', not %r" % (direction,))
    if not float(radius) > 0.0:
        raise ValueError("radius must be > 0")
    if int(offset) != offset or int(offset) < 0:
        raise ValueError("offset must be an integer >= 0")
    return {"radius": float(radius), "offset": int(offset), "connect": connect, "direction": direction}


def hse_raw(api, xyz, atom_ptr, res_ptr, bb, target_res, target_complex, radius=12.0, offset=0, connect="CA",
            direction="CA", device="cpu", tile=None, keep_device=False):
    """One drgnn_hse_residues call (include/drgnn.h) over numpy arrays; the targets in any order (they are grouped by
    complex and cut into tiles of ``tile``, default ``hse_tile``, here, and the rows come back in the order asked for).
    ``connect``: "CA", "CN" or (column, column, cutoff).  Returns (out float64 [K,3]: up, down, angle, NaN rows for no value; status int): bit 0
    of status says a complex was beyond the capacity (its rows are NaN).  ``keep_device``: ``out`` stays a tensor on
    ``device``; only the status word comes back."""
    dev = torch.device(device)
    con = HSE_CONNECT[connect] if isinstance(connect, str) else connect
    tgt_res = np.asarray(target_res, dtype=np.int64).reshape(-1)
    tgt_cx = np.asarray(target_complex, dtype=np.int64).reshape(-1)
    if tgt_res.shape != tgt_cx.shape:
        raise ValueError("the two target arrays must have one length")
    K = int(tgt_res.shape[0])
    tile = max(1, int(tile or hse_tile(K)))
    order = np.argsort(tgt_cx, kind="stable")
    sorted_cx = tgt_cx[order]
    first = np.flatnonzero(np.concatenate(([True], sorted_cx[1:] != sorted_cx[:-1]))) if K else np.zeros(0, np.int64)
    ends = np.append(first[1:], K)
    cuts = [np.arange(lo, hi, tile) for lo, hi in zip(first, ends)]
    tile_ptr = np.concatenate(cuts + [np.array([K])])
    bb = np.ascontiguousarray(bb, dtype=np.int32).reshape(-1, 5)
    host = [np.ascontiguousarray(a, dtype=np.int32) for a in (atom_ptr, res_ptr, bb, tgt_res[order], sorted_cx, tile_ptr)]
    d_xyz = torch.from_numpy(np.ascontiguousarray(xyz, dtype=np.float32).reshape(-1, 3)).to(dev)
    if api is _lib._API:
        _lib.require_device(d_xyz)
    d_host = [torch.from_numpy(h).to(dev) for h in host]
    out = torch.empty((K, 3), dtype=torch.float64, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    q = _lib.HseRequest()
    q.xyz = d_xyz.data_ptr()
    q.atom_ptr, q.res_ptr, q.bb, q.target_res, q.target_complex, q.tile_ptr = [t.data_ptr() for t in d_host]
    (q.host_atom_ptr, q.host_res_ptr, q.host_bb, q.host_target_res, q.host_target_complex,
     q.host_tile_ptr) = [h.ctypes.data for h in host]
    q.n_atoms, q.n_residues, q.n_complexes = int(d_xyz.shape[0]), len(host[0]) - 1, len(host[1]) - 1
    q.n_targets, q.n_tiles, q.n_rows = K, len(tile_ptr) - 1, int(bb.shape[0])
    q.radius, q.offset, q.direction = float(radius), int(offset), HSE_DIRECTION.get(direction, direction)
    q.connect_a, q.connect_b, q.connect_cutoff = int(con[0]), int(con[1]), float(con[2])
    q.out, q.status = out.data_ptr(), status.data_ptr()
    api.hse_residues(q, _lib.current_stream(d_xyz))
    if keep_device:
        if not np.array_equal(order, np.arange(K)):                        # (targets listed complex by complex: as they are)
            rows = torch.empty_like(out)
            rows[torch.from_numpy(order).to(dev)] = out
            out = rows
        return out, int(status.cpu()[0])
    rows = np.empty((K, 3))
    rows[order] = out.cpu().numpy()
    return rows, int(status.cpu()[0])


def residue_hse(tables_or_poses, residues=None, radius=12.0, offset=0, connect="CA", direction="CA", device=None, chunk=None,
                api=None):
    """Half-sphere exposure of residues, on the device: (up, down, angle) as the reference's ``hse`` node feature
    records it from Biopython's ``HSExposureCA(model)`` (``radius`` 12 A, ``offset`` 0).  The CA trace is cut into
    peptides: consecutive standard residues of a chain are linked when their CAs are closer than 4.3 A (``connect``
    "CA", Biopython's CaPPBuilder) or the C of one and the N of the next closer than 1.8 A ("CN", its PPBuilder).  A
    residue linked on both sides has a value: ``up`` / ``down`` count the CAs of the other linked residues within
    ``radius`` on either side of the plane through its CA whose normal is the sum of the unit vectors from its two
    neighbours' CAs; ``angle`` (rad) lies between that normal and CA -> CB (a GLY: the N turned by -120 degrees about CA
    -> C).  ``offset`` k also leaves out the residues of the same peptide at most k positions away.
    ``direction`` "CB" is Biopython's ``HSExposureCB``: the normal is CA -> CB itself, every linked residue with that
    vector has a value and the angle is 0 (the reference records nothing for it: it is held to the written rule of
    tests/hse_ref.py alone).

    An ``AtomTable`` gives float64 [R,3], an ``AtomTable.poses`` batch [M,R,3], a sequence of either a list of [R_k,3];
    NaN rows mark residues without a value and residues not asked for.  ``residues``: None (all), an index array
    applied to every complex, or one index array per complex.  ``chunk``: complexes per launch; a residue's bits do
    not depend on it, on the batch or on ``residues``.  The tables must have been made with ``atom_name``.  A complex of
    more than 4096 residues is refused (DrgnnError, capacity)."""
    return _residue_values(HSE, tables_or_poses, residues, None,
                           {"radius": radius, "offset": offset, "connect": connect, "direction": direction}, device, chunk, api)


# ---- residue depth (csrc/drgnn_depth.h) --------------------------------------------------------------------------------
DEPTH_UNITED = {"C": 1.9, "N": 1.7, "O": 1.5, "S": 1.85, "H": 0.0}     # MSMS' united-atom radii by the first letter of the name
DEPTH_OTHER = 1.8                                                      # any other first letter
DEPTH_COMPONENTS = {"outer": 0, "all": 1}
# bytes of workspace one drgnn_depth_residues call may ask for (sets the complexes per call): k_depth_components gives a
# complex one workgroup, so a call on the device should hold about as many complexes as there are compute units (256;
# 1ATN at 192 dots: 41.7 MB each); the host emulation runs them one after the other
DEPTH_WORKSPACE_BUDGET = {"cpu": 1 << 30, "cuda": 13 << 30}


def depth_radii(table, radii="united"):
    """float64 [T] in the table's grouped atom order; 0: the atom takes no part in the surface.  "united": MSMS'
    united-atom radii by the first letter of the atom name (C 1.9, N 1.7, O 1.5, S 1.85, H 0, any other letter 1.8); a
    name without a letter raises ValueError.  An array [n_input_atoms] in input atom order is taken as
    it is."""
    if isinstance(radii, str):
        if radii != "united":
            raise ValueError("radii must be 'united' or an array, not %r" % radii)
        if table.atom_name is None:
            raise ValueError("the radius table goes by atom name: build the AtomTable with atom_name=")
        out = np.empty(table.n_atoms)
        for i, nm in enumerate(table.atom_name):
            letters = [ch for ch in str(nm) if ch.isalpha()]
            if not letters:
                raise ValueError("no radius for the atom name %r: it holds no letter" % str(nm))
            out[i] = DEPTH_UNITED.get(letters[0], DEPTH_OTHER)
        return out
    a = np.asarray(radii, dtype=np.float64)
    if a.shape != (table.n_input_atoms,):
        raise ValueError("the radius array needs %d entries, one per input atom" % table.n_input_atoms)
    if not np.all(a >= 0.0):                                           # (NaN fails too)
        raise ValueError("radii must be >= 0 (0: the atom takes no part in the surface)")
    return a[table.order]


def depth_dots(n_dots):
    """float64 [n_dots, 3]: the unit dots S_k = (rho cos phi, rho sin phi, z), z = 1 - (2k + 1) / n, rho = sqrt(1 - z^2),
    phi = (k + 1/2) pi (3 - sqrt 5), as tests/depth_ref.py writes them"""
    k = np.arange(int(n_dots), dtype=np.float64)
    z = 1.0 - (2.0 * k + 1.0) / int(n_dots)
    rho = np.sqrt(1.0 - z * z)
    phi = (k + 0.5) * (np.pi * (3.0 - np.sqrt(5.0)))
    return np.stack((rho * np.cos(phi), rho * np.sin(phi), z), axis=1)


def depth_link(n_dots, probe=1.5):
    """the default link length: one and a half dot spacings on a sphere of radius 1.8 + probe"""
    return float(1.5 * np.sqrt(4.0 * np.pi * (DEPTH_OTHER + probe) ** 2 / int(n_dots)))


def _depth_options(probe=1.5, n_dots=192, link=None, components="outer"):
    if int(n_dots) != n_dots or int(n_dots) < 1:
        raise ValueError("n_dots must be an integer >= 1")
    if not float(probe) > 0.0 or not np.isfinite(float(probe)):
        raise ValueError("probe must be > 0")
    if components not in DEPTH_COMPONENTS:
        raise ValueError("components must be 'outer' or 'all', not %r" % (components,))
    link = depth_link(n_dots, float(probe)) if link is None else float(link)
    if not link >= 0.0 or not np.isfinite(link):
        raise ValueError("link must be >= 0")
    return {"probe": float(probe), "n_dots": int(n_dots), "link": link, "components": components}


def depth_raw(api, xyz, atom_ptr, res_ptr, radii, target_res, target_complex, probe=1.5, n_dots=192, link=None,
              components="outer", device="cpu", keep_device=False, parts=False):
    """One drgnn_depth_residues call (include/drgnn.h) over numpy arrays.  Returns (out float64 [K], status int): bit 0 of
    status says a complex was beyond the capacity (its targets are NaN).  ``keep_device``: ``out`` stays a tensor on
    ``device``.  ``parts``: a third value, the surface the call left in its workspace, per complex a dict of ``mask`` bool
    [atoms, n_dots], ``ids`` (dot ids atom n_dots + k of the accessible dots, atoms counted within the complex),
    ``label`` (the smallest dot id of each dot's component) and ``outer`` (the label kept; -1: all or none)."""
    dev = torch.device(device)
    link = depth_link(n_dots, probe) if link is None else float(link)
    host = [np.ascontiguousarray(a, dtype=np.int32).reshape(-1) for a in (atom_ptr, res_ptr, target_res, target_complex)]
    if host[2].shape != host[3].shape:
        raise ValueError("the two target arrays must have one length")
    rad = np.ascontiguousarray(radii, dtype=np.float64).reshape(-1)
    d_xyz = torch.from_numpy(np.ascontiguousarray(xyz, dtype=np.float32).reshape(-1, 3)).to(dev)
    if api is _lib._API:
        _lib.require_device(d_xyz)
    T, M, K = int(d_xyz.shape[0]), len(host[1]) - 1, int(host[2].shape[0])
    d_host = [torch.from_numpy(h).to(dev) for h in host]
    d_rad = torch.from_numpy(rad).to(dev)
    d_dots = torch.from_numpy(depth_dots(n_dots)).to(dev)
    n_bytes, off = api.depth_workspace(T, M, n_dots)
    work = torch.empty(max(1, n_bytes // 8), dtype=torch.int64, device=dev)
    out = torch.empty(K, dtype=torch.float64, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    q = _lib.DepthRequest()
    q.xyz, q.radii, q.dots = d_xyz.data_ptr(), d_rad.data_ptr(), d_dots.data_ptr()
    q.atom_ptr, q.res_ptr, q.target_res, q.target_complex = [t.data_ptr() for t in d_host]
    q.host_atom_ptr, q.host_res_ptr, q.host_target_res, q.host_target_complex = [h.ctypes.data for h in host]
    q.n_atoms, q.n_residues, q.n_complexes, q.n_targets, q.n_radii = T, len(host[0]) - 1, M, K, int(rad.shape[0])
    q.probe, q.link, q.n_dots, q.components = float(probe), link, int(n_dots), DEPTH_COMPONENTS.get(components, components)
    q.workspace, q.workspace_bytes = work.data_ptr(), n_bytes
    q.out, q.status = out.data_ptr(), status.data_ptr()
    api.depth_residues(q, _lib.current_stream(d_xyz))
    result = (out if keep_device else out.cpu().numpy()), int(status.cpu()[0])
    if not parts:
        return result
    w = work.cpu().numpy().view(np.uint8)
    W, D = (int(n_dots) + 63) // 64, T * int(n_dots)
    mask = w[off[0]:off[0] + 8 * T * W].view(np.uint64).reshape(T, W)
    bits = ((mask[:, :, None] >> np.arange(64, dtype=np.uint64)[None, None, :]) & np.uint64(1)).astype(bool)
    bits = bits.reshape(T, W * 64)[:, :int(n_dots)]
    ids, label = (w[off[j]:off[j] + 4 * D].view(np.int32) for j in (2, 3))
    cx_nd, cx_outer = (w[off[j]:off[j] + 4 * M].view(np.int32) for j in (7, 8))
    first = host[0][host[1]]                                           # the first atom of every complex
    surf = []
    for c in range(M):
        a0, a1, nd = int(first[c]), int(first[c + 1]), int(cx_nd[c])
        base = a0 * int(n_dots)
        if K == 0 or cx_outer[c] == -2:
            surf.append(None)
            continue
        cid = ids[base:base + nd].astype(np.int64)
        surf.append({"mask": bits[a0:a1].copy(), "ids": cid, "label": cid[label[base:base + nd]],
                     "outer": int(cid[cx_outer[c]]) if cx_outer[c] >= 0 else -1})
    return result + (surf,)


def _depth_too_large(api, part, residues, opt, device):
    """a call of these complexes is beyond the workspace budget or the grid"""
    atoms = sum(t.n_atoms for t, _ in part)
    budget = DEPTH_WORKSPACE_BUDGET["cuda" if torch.device(device).type == "cuda" else "cpu"]
    return (44 * atoms * opt["n_dots"] > budget or
            max(sum(len(r) for r in residues), len(part), atoms // 16 + 1) > api.depth_capacity(2))


def residue_depth(tables_or_poses, residues=None, radii="united", probe=1.5, n_dots=192, link=None, components="outer",
                  device=None, chunk=None, api=None):
    """Residue depth (A), on the device: the mean, over the atoms of a residue, of the distance to the molecular surface
    of the complex, as the reference's ``depth`` node feature records it from Biopython's ``residue_depth`` (MSMS).
    MSMS is not reproduced: the surface is a dot surface of the solvent-accessible surface of all atoms of both chains
    (``n_dots`` golden-spiral dots on every sphere of radius r + ``probe``; see ``depth_radii`` for ``radii``), restricted
    to its outer component (dots closer than ``link`` are linked, default one and a half dot spacings; the component with
    the most dots is kept, so that cavities do not count), and depth(atom) = distance to the nearest kept dot - ``probe``.
    ``components`` "all" keeps every accessible dot (for comparison).  tests/depth_ref.py states the rule; on the 496
    recorded 1ATN nodes it lies within 0.15 A rms of the reference's values (r = 0.990), one MSMS vertex spacing.  The
    dot lattice is fixed in the frame of the input: the value is not invariant under rotation, it varies within the dot
    spacing.

    An ``AtomTable`` gives float64 [R], an ``AtomTable.poses`` batch [M, R], a sequence of either a list of [R_k], with
    NaN for the residues not asked for.  ``residues``: None (all), an index array applied to every complex, or one
    index array per complex.  ``chunk``: complexes per call (the workspace also bounds it); a residue's bits do not
    depend on it, on the batch or on ``residues``.  The tables must have been made with ``atom_name``.  More than 4096
    dots per atom, or a complex of more than 4 194 304 atoms x n_dots, is refused (DrgnnError, capacity)."""
    return _residue_values(DEPTH, tables_or_poses, residues, radii,
                           {"probe": probe, "n_dots": n_dots, "link": link, "components": components}, device, chunk, api)


# ---- the per-residue features: one record each, one path for all ("Per-residue features") --------------------
# name: of the option, of node_data/<name> and of the node feature;  row: the shape of one row of the raw call's out
# check(**options): the options of the raw call, validated;  host_table(table, radii): the arrays the raw call takes per
# table, a tuple;  ragged: how many of (xyz, atom_ptr, res_ptr, res_split) the raw call takes;  raw: one call of the
# library;  too_large(api, part, residues, opt, device): the call must be halved;  c_name: the entry point, for errors
# options(value, tables): the graph paths' option (True, a dict, a radii value) as (opt, host tables by id(table))
# needs: what, besides True, the option may be;  node_data(rows): the rows of a complex as the store keeps them
# pack: the (source, column) pairs of drgnn_iface_pack, which takes the rows as the argument ``name``
Feature = collections.namedtuple("Feature", "name row check host_table ragged raw too_large c_name options needs node_data pack")


def _per_table(feature, tables, radii):
    """{id(table): host arrays}: each distinct table's, made once"""
    found = {}
    for t in tables:
        if id(t) not in found:
            found[id(t)] = feature.host_table(t, radii)
    return found


def _bsa_graph_options(value, tables):
    return {"probe": 1.4, "n_slices": 20}, _per_table(BSA, tables, "reference" if value is True else value)


def _hse_graph_options(value, tables):
    opt = _hse_options(**({} if value is True else dict(value)))
    return opt, _per_table(HSE, tables, None)


def _depth_graph_options(value, tables):
    opt = dict({} if value is True else value)
    tabs_of = _per_table(DEPTH, tables, opt.pop("radii", "united"))
    return _depth_options(**opt), tabs_of


def _hse_node_data(rows):
    rows = rows.copy()
    rows[np.isnan(rows[:, 0])] = 0.0
    return rows


BSA = Feature(name="bsa", row=(3,), check=_bsa_options, host_table=bsa_radii, ragged=4, raw=bsa_raw,
              # one workgroup per target: the grid's limit
              too_large=lambda api, part, residues, opt, device: sum(len(r) for r in residues) > api.bsa_capacity(3),
              c_name="drgnn_bsa_residues", options=_bsa_graph_options, needs="a radii option",
              node_data=lambda rows: rows[:, 2:3].copy(), pack=[(_lib.PACK_BSA, 2)])
HSE = Feature(name="hse", row=(3,), check=_hse_options, host_table=lambda table, radii: (hse_table(table),), ragged=3, raw=hse_raw,
              # one workgroup per tile
              too_large=lambda api, part, residues, opt, device: (sum(len(r) // HSE_TILE[0] + 1 for r in residues) >
                                                                  api.hse_capacity(1)),
              c_name="drgnn_hse_residues", options=_hse_graph_options, needs="a dict of options",
              node_data=_hse_node_data, pack=[(_lib.PACK_HSE, j) for j in range(3)])
DEPTH = Feature(name="depth", row=(), check=_depth_options, host_table=lambda table, radii: (depth_radii(table, radii),),
                ragged=3, raw=depth_raw, too_large=_depth_too_large,
                c_name="drgnn_depth_residues", options=_depth_graph_options, needs="a dict of options",
                node_data=lambda rows: rows.copy(), pack=[(_lib.PACK_DEPTH, 0)])
FEATURES = (BSA, HSE, DEPTH)                                           # in the order of the options of the graph paths
PACK_SOURCE.update({f.name: f.pack for f in FEATURES})
FEATURE_WIDTH = {name: len(cols) for name, cols in PACK_SOURCE.items()}    # columns of x behind every built-in node feature


def _targets(residues, res_ptr):
    """(target_res, target_complex, sizes) of per-complex lists of local residue indices"""
    sizes = [len(r) for r in residues]
    tgt_res = np.concatenate([np.asarray(r, dtype=np.int64) + int(res_ptr[k]) for k, r in enumerate(residues)]
                             + [np.zeros(0, np.int64)])
    return tgt_res, np.repeat(np.arange(len(residues)), sizes), sizes


def _feature_chunk(feature, api, part, residues, tabs_of, opt, device, ragged=None, keep_device=False):
    """[rows float64 [K_c] + feature.row] for the complexes of ``part`` ([(table, xyz)]) and their residue lists (local
    indices); ``ragged``: ``_ragged(part)`` when the caller has it.  ``keep_device``: one tensor [sum K_c] + feature.row
    on ``device`` instead, the complexes' rows back to back."""
    if len(part) > 1 and feature.too_large(api, part, residues, opt, device):
        half = len(part) // 2
        both = [_feature_chunk(feature, api, part[h], residues[h], tabs_of, opt, device, keep_device=keep_device)
                for h in (slice(0, half), slice(half, None))]
        return torch.cat(both) if keep_device else both[0] + both[1]
    ragged = (ragged if ragged is not None else _ragged(part))[:feature.ragged]
    tables = [t for t, _ in part]
    if all(t is tables[0] for t in tables):                              # poses of one topology share one table
        tabs = tabs_of[id(tables[0])]
    else:
        tabs = [np.concatenate(arrays) for arrays in zip(*[tabs_of[id(t)] for t in tables])]
    tgt_res, tgt_cx, sizes = _targets(residues, ragged[2])
    out, status = feature.raw(api, *ragged, *tabs, tgt_res, tgt_cx, device=device, keep_device=keep_device, **opt)
    if status & 1:
        _lib._check(-2, feature.c_name)
    if keep_device:
        return out
    ends = np.cumsum(sizes)
    return [out[e - n:e] for n, e in zip(sizes, ends)]


def _residue_values(feature, tables_or_poses, residues, radii, options, device, chunk, api):
    """``residue_bsa`` / ``residue_hse`` / ``residue_depth``: the raw rows of the residues asked for, NaN elsewhere; an
    ``AtomTable`` gives float64 [R] + feature.row, an ``AtomTable.poses`` batch [M, R] + feature.row, a sequence a list"""
    api = api or _lib.get()
    device = _default_device(api, device)
    cx = _complexes(tables_or_poses)
    opt = feature.check(**options)
    tabs_of = _per_table(feature, [t for t, _ in cx], radii)
    if residues is None:
        wanted = [np.arange(t.n_residues) for t, _ in cx]
    else:
        per_complex = (isinstance(residues, (list, tuple)) and len(residues) == len(cx) and
                       all(np.ndim(r) == 1 for r in residues))
        wanted = [np.asarray(residues[k] if per_complex else residues, dtype=np.int64).reshape(-1) for k in range(len(cx))]
        for (t, _), w in zip(cx, wanted):
            if w.size and (w.min() < 0 or w.max() >= t.n_residues):
                raise ValueError("a residue index outside [0, %d)" % t.n_residues)
    if chunk is None:
        chunk = RESIDUE_XYZ_BUDGET // (12 * max([t.n_atoms for t, _ in cx] + [1]))
    chunk = max(1, int(chunk))
    full = [np.full((t.n_residues,) + feature.row, np.nan) for t, _ in cx]
    for lo in range(0, len(cx), chunk):
        part = cx[lo:lo + chunk]
        for k, o in enumerate(_feature_chunk(feature, api, part, wanted[lo:lo + chunk], tabs_of, opt, device)):
            full[lo + k][wanted[lo + k]] = o
    if isinstance(tables_or_poses, AtomTable):
        return full[0]
    if isinstance(tables_or_poses, Poses):
        return np.stack(full) if full else np.zeros((0, tables_or_poses.table.n_residues) + feature.row)
    return full


# ---- clustering of poses by their fraction of common contacts (csrc/drgnn_fcc.h) -----------------------------------
FCC_XYZ_BUDGET = 256 << 20         # bytes of pose coordinates one drgnn_pose_contacts call uploads (sets the default chunk)


def counted_atoms(table, heavy_only=None):
    """(keep int64 [T'], atom_ptr int32 [R+1]): the atoms of ``table`` (grouped order) that decide contacts and their
    grouping into residues.  ``heavy_only``: leave out hydrogens, the atoms whose name's first character that is neither a
    digit nor a blank is ``H``; None: True when the table has atom names."""
    if heavy_only is None:
        heavy_only = table.atom_name is not None
    keep = np.ones(table.n_atoms, dtype=bool)
    if heavy_only:
        if table.atom_name is None:
            raise ValueError("heavy_only=True finds hydrogens by atom name: build the AtomTable with atom_name=")
        keep = np.array([n.lstrip("0123456789 ")[:1] != "H" for n in table.atom_name], dtype=bool).reshape(-1)
    res_of_atom = np.repeat(np.arange(table.n_residues), np.diff(table.atom_ptr))
    counts = np.bincount(res_of_atom[keep], minlength=table.n_residues)
    return np.flatnonzero(keep), np.concatenate(([0], np.cumsum(counts))).astype(np.int32)


def _pose_batch(poses, table, mismatch="the poses must be of the given AtomTable"):
    """(table, xyz float32 [M, T, 3] in the table's grouped order) of an ``AtomTable.poses`` batch, a table, or xyz with
    ``table``; ``mismatch``: what to say of a batch or table that is not ``table``"""
    if isinstance(poses, (Poses, AtomTable)):
        own = poses.table if isinstance(poses, Poses) else poses
        if table is not None and own is not table:
            raise ValueError(mismatch)
        return own, (poses.xyz if isinstance(poses, Poses) else poses.xyz[None])
    if table is None:
        raise ValueError("coordinates need table=, the AtomTable they are poses of")
    xyz = np.asarray(poses)
    if xyz.ndim != 3 or xyz.shape[1:] != (table.n_atoms, 3):
        raise ValueError("poses need xyz [M, %d, 3]" % table.n_atoms)
    return table, xyz


class PoseContacts(object):
    """``pose_contacts``: ``bits`` int64 [M, nA, WB] on the device (the 64-bit words of drgnn_pose_contacts: bit b % 64
    of word b / 64 of row a says that residue a of the first chain and residue b of the second are in contact),
    ``n_contacts`` int64 [M] on the host, ``table``, ``n_a`` / ``n_b`` the residues of the two chains."""

    def __init__(self, table, bits, n_contacts, api, device, cutoff, heavy_only):
        self.table, self.bits, self.n_contacts, self.api, self.device = table, bits, n_contacts, api, device
        self.cutoff, self.heavy_only = cutoff, heavy_only
        self.n_a, self.n_b = table.split, table.n_residues - table.split

    def __len__(self):
        return int(self.n_contacts.shape[0])

    def words(self, m=None):
        """the words as numpy uint64 [M, nA, WB], or [nA, WB] of pose m"""
        w = (self.bits if m is None else self.bits[m]).cpu().numpy().view(np.uint64)
        return w

    def pairs(self, m):
        """int32 [n_m, 2]: the contacts of pose m as (residue of the first chain, residue of the second), both indices
        into the table's residues, sorted"""
        if self.n_a == 0 or self.n_b == 0:
            return np.zeros((0, 2), np.int32)
        w = self.words(m)
        on = np.unpackbits(w.view(np.uint8).reshape(self.n_a, -1), axis=1, bitorder="little")[:, :self.n_b]
        a, b = np.nonzero(on)
        return np.stack((a, b + self.n_a), axis=1).astype(np.int32)

    def select(self, index):
        """the ``PoseContacts`` of the poses ``index`` (int [K], in that order; a pose may repeat), its bits gathered on
        the device: what carries the best few thousand of a large set into ``cluster_poses``"""
        idx = np.asarray(index)
        if idx.dtype == bool or idx.ndim != 1 or (idx.size and not np.issubdtype(idx.dtype, np.integer)):
            raise ValueError("index must be a list of pose indices")
        idx = idx.astype(np.int64)
        if idx.size and (idx.min() < 0 or idx.max() >= len(self)):
            raise ValueError("index must lie in [0, %d)" % len(self))
        bits = self.bits.index_select(0, torch.from_numpy(idx).to(self.bits.device))
        return PoseContacts(self.table, bits, self.n_contacts[idx], self.api, self.device, self.cutoff, self.heavy_only)


def pose_contacts_raw(api, xyz, atom_ptr, n_chain_a, cutoff=5.0, device="cpu"):
    """One drgnn_pose_contacts call (include/drgnn.h) over numpy arrays: xyz float32 [M, T, 3] of the counted atoms.
    Returns (bits int64 [M, nA, WB], n_contacts int32 [M]) as tensors on ``device``."""
    dev = torch.device(device)
    xyz = np.ascontiguousarray(xyz, dtype=np.float32)
    host = np.ascontiguousarray(atom_ptr, dtype=np.int32)
    M, R, nA = int(xyz.shape[0]), len(host) - 1, int(n_chain_a)
    d_xyz = torch.from_numpy(xyz).to(dev)
    if api is _lib._API:
        _lib.require_device(d_xyz)
    d_ap = torch.from_numpy(host).to(dev)
    bits = torch.empty((M, max(nA, 0), (max(R - nA, 0) + 63) // 64), dtype=torch.int64, device=dev)
    count = torch.empty(M, dtype=torch.int32, device=dev)
    q = _lib.PoseContactsRequest()
    q.xyz, q.atom_ptr, q.host_atom_ptr = d_xyz.data_ptr(), d_ap.data_ptr(), host.ctypes.data
    q.n_poses, q.n_atoms, q.n_residues, q.n_chain_a, q.cutoff = M, int(xyz.shape[1]), R, nA, float(cutoff)
    q.bits, q.n_contacts = bits.data_ptr(), count.data_ptr()
    api.pose_contacts(q, _lib.current_stream(d_xyz))
    return bits, count


def pose_contacts(poses, cutoff=5.0, heavy_only=None, device=None, api=None, chunk=None, table=None):
    """The interface contacts of M poses of one topology (an ``AtomTable.poses`` batch, a table, or xyz float32 [M,T,3]
    in the grouped atom order of ``table``), on the device: residue a of the first chain and residue b of the second are
    in contact when a counted atom of each lie within ``cutoff`` A (d^2 <= float32(cutoff^2) on the float32 coordinates,
    the rule of ``fnat``).  ``heavy_only``: hydrogens do not count (the default when the table has atom names).  Returns a
    ``PoseContacts``; a pose's bits do not depend on M, on ``chunk`` (poses per launch), on its place or on the run."""
    if not float(cutoff) > 0.0 or not float(cutoff) < 1e18:
        raise ValueError("cutoff must be > 0")
    t, xyz = _pose_batch(poses, table)
    keep, atom_ptr = counted_atoms(t, heavy_only)
    api = api or _lib.get()
    device = _default_device(api, device)
    if t.n_residues > api.fcc_capacity(0):
        _lib._check(-2, "drgnn_pose_contacts")
    if chunk is None:
        chunk = FCC_XYZ_BUDGET // (12 * max(len(keep), 1))
    chunk = max(1, int(chunk))
    nA, WB = t.split, (t.n_residues - t.split + 63) // 64
    parts = [pose_contacts_raw(api, xyz[lo:lo + chunk][:, keep], atom_ptr, nA, cutoff, device)
             for lo in range(0, xyz.shape[0], chunk)]
    if parts:
        bits = torch.cat([p[0] for p in parts]) if len(parts) > 1 else parts[0][0]
        count = np.concatenate([p[1].cpu().numpy() for p in parts]).astype(np.int64)
    else:
        bits, count = torch.empty((0, nA, WB), dtype=torch.int64, device=torch.device(device)), np.zeros(0, np.int64)
    return PoseContacts(t, bits, count, api, device, float(cutoff), len(keep) != t.n_atoms)


def pose_common_raw(api, bits_a, bits_b):
    """One drgnn_pose_common call over tensors of words [Ma, W] and [Mb, W] (one device): int32 [Ma, Mb] on that device"""
    Ma, Mb, W = int(bits_a.shape[0]), int(bits_b.shape[0]), int(bits_a.shape[1])
    out = torch.empty((Ma, Mb), dtype=torch.int32, device=bits_a.device)
    q = _lib.PoseCommonRequest()
    q.bits_a, q.bits_b, q.common = bits_a.data_ptr(), bits_b.data_ptr(), out.data_ptr()
    q.n_a, q.n_b, q.n_words = Ma, Mb, W
    api.pose_common(q, _lib.current_stream(bits_a))
    return out


def _blocked_pairs(raw, A, B, block, dtype, symmetric=False):
    """``raw(rows of A, rows of B)`` over blocks of at most ``block`` rows a side, as one tensor [len(A), len(B)].
    ``symmetric`` (B is A): a diagonal block gets one tensor object as both sides, a block above the diagonal is computed
    once and mirrored by ``.t()``"""
    if len(A) <= block and len(B) <= block:
        return raw(A, B)
    out = torch.empty((len(A), len(B)), dtype=dtype, device=A.device)
    for i in range(0, len(A), block):
        for j in range(i if symmetric else 0, len(B), block):
            rows = A[i:i + block]
            part = raw(rows, rows if symmetric and j == i else B[j:j + block])
            out[i:i + block, j:j + block] = part
            if symmetric and j > i:
                out[j:j + block, i:i + block] = part.t()
    return out


def _common_device(a, b=None):
    """common contacts of two ``PoseContacts`` as an int32 tensor [M, M2] on their device; calls of at most
    drgnn_fcc_capacity(1) poses a side"""
    b = a if b is None else b
    if not isinstance(a, PoseContacts) or not isinstance(b, PoseContacts):
        raise ValueError("common contacts are taken between PoseContacts (pose_contacts)")
    if (a.n_a, a.n_b) != (b.n_a, b.n_b) or a.api is not b.api or torch.device(a.device) != torch.device(b.device):
        raise ValueError("the two sets of contacts must be of one topology, library and device")
    W = a.n_a * ((a.n_b + 63) // 64)
    wa, wb = a.bits.reshape(len(a), W), b.bits.reshape(len(b), W)
    if len(a) == 0 or len(b) == 0:
        return torch.zeros((len(a), len(b)), dtype=torch.int32, device=wa.device)
    return _blocked_pairs(lambda x, y: pose_common_raw(a.api, x, y), wa, wb, a.api.fcc_capacity(1), torch.int32)


def common_contacts(a, b=None):
    """int32 [M, M2]: the number of contacts pose i of ``a`` shares with pose j of ``b`` (``b`` None: of ``a`` itself; the
    diagonal is then ``n_contacts``).  ``a`` and ``b`` are ``PoseContacts`` of one topology."""
    return _common_device(a, b).cpu().numpy()


def fcc_matrix(a, b=None):
    """float64 [M, M2]: the fraction of the contacts of pose i of ``a`` that pose j of ``b`` has too, ``common[i, j] /
    n_contacts[i]`` as one float64 division; a pose without contacts has a row of zeros.  Not symmetric."""
    common = common_contacts(a, b).astype(np.float64)
    n = a.n_contacts.astype(np.float64)
    out = np.zeros_like(common)
    has = n > 0
    out[has] = common[has] / n[has, None]
    return out


class PoseClusters(object):
    """``cluster_poses``: ``labels`` int64 [M] (the cluster of every pose in order of discovery, -1: in none),
    ``centres`` / ``sizes`` int64 [K] per cluster, ``n_contacts`` int64 [M] (None from ``cluster_poses_rmsd``)."""

    def __init__(self, labels, centres, sizes, n_contacts):
        self.labels, self.centres, self.sizes, self.n_contacts = labels, centres, sizes, n_contacts

    def __len__(self):
        return int(self.centres.shape[0])

    def rank(self, scores, top=4, ascending=False):
        """(order int64 [K], means float64 [K]): the clusters ordered by the mean of their ``top`` best member scores
        (HADDOCK's convention; all members of a smaller cluster), best first, ties by cluster ordinal; ``means`` per
        cluster ordinal.  ``scores`` [M]: what ``Ensemble.predict`` or ``docking_scores()[key]`` gives for the same
        poses; ``ascending``: the smaller score is the better one."""
        if torch.is_tensor(scores):
            scores = scores.detach().cpu().numpy()
        scores = np.asarray(scores, dtype=np.float64).reshape(-1)
        if scores.shape[0] != self.labels.shape[0]:
            raise ValueError("%d scores for %d poses" % (scores.shape[0], self.labels.shape[0]))
        if int(top) < 1:
            raise ValueError("top must be >= 1")
        means = np.zeros(len(self))
        for k in range(len(self)):
            s = np.sort(scores[self.labels == k])
            means[k] = (s if ascending else s[::-1])[:int(top)].mean()
        order = np.lexsort((np.arange(len(self)), means if ascending else -means))
        return order.astype(np.int64), means

    def consensus(self, contacts):
        """the ``ContactFrequency`` of every cluster: ``contact_frequency(contacts, groups=self.labels,
        n_groups=len(self))`` for the ``PoseContacts`` of the clustered poses"""
        if not isinstance(contacts, PoseContacts):
            raise ValueError("a consensus is taken from PoseContacts (pose_contacts)")
        if len(contacts) != self.labels.shape[0]:
            raise ValueError("%d poses for %d labels" % (len(contacts), self.labels.shape[0]))
        return contact_frequency(contacts, groups=self.labels, n_groups=len(self))


def _cluster_launch(api, call, q, rows, min_size):
    """One clustering call, whatever the rule (csrc/drgnn_posecluster.h): ``q`` holds the rule's own fields and ``rows``
    is one of its inputs on the device, a row per pose; this adds the shared fields and the outputs, runs ``call`` (the
    entry point) and returns the dict ``pose_cluster_raw`` documents"""
    if api is _lib._API:
        _lib.require_device(rows)
    M = int(rows.shape[0])
    nb = torch.zeros((2, M, (M + 63) // 64), dtype=torch.int64, device=rows.device)
    res = torch.zeros((3, M), dtype=torch.int32, device=rows.device)
    k = torch.zeros(1, dtype=torch.int32, device=rows.device)
    q.n_poses, q.min_size = M, int(min_size)
    q.neighbours, q.transposed = nb[0].data_ptr(), nb[1].data_ptr()
    q.labels, q.centres, q.sizes, q.n_clusters = res[0].data_ptr(), res[1].data_ptr(), res[2].data_ptr(), k.data_ptr()
    call(q, _lib.current_stream(rows))
    K = int(k.cpu()[0])
    res, nb = res.cpu().numpy(), nb.cpu().numpy().view(np.uint64)
    return {"labels": res[0].copy(), "centres": res[1, :K].copy(), "sizes": res[2, :K].copy(), "neighbours": nb[0].copy(),
            "transposed": nb[1].copy()}


def _check_min_size(min_size):
    if int(min_size) != min_size or int(min_size) < 1:
        raise ValueError("min_size must be an integer >= 1")


def _pose_clusters(r, n_contacts):
    """the ``PoseClusters`` of a raw result (None: of no poses)"""
    r = r or dict.fromkeys(("labels", "centres", "sizes"), np.zeros(0, np.int32))
    return PoseClusters(r["labels"].astype(np.int64), r["centres"].astype(np.int64), r["sizes"].astype(np.int64), n_contacts)


def pose_cluster_raw(api, common, n_contacts, cutoff_fcc=0.6, cutoff_reverse=0.45, min_size=4, device="cpu"):
    """One drgnn_pose_cluster call (include/drgnn.h): ``common`` int32 [M, M] and ``n_contacts`` int32 [M] as numpy arrays
    or tensors on ``device``.  Returns a dict of numpy arrays: labels int32 [M], centres / sizes int32 [K], neighbours /
    transposed uint64 [M, ceil(M/64)] (the directed relation and its transpose as bit rows)."""
    dev = torch.device(device)
    d_c = common if torch.is_tensor(common) else torch.from_numpy(np.ascontiguousarray(common, dtype=np.int32)).to(dev)
    d_n = (n_contacts if torch.is_tensor(n_contacts) else
           torch.from_numpy(np.ascontiguousarray(n_contacts, dtype=np.int32)).to(dev))
    d_c, d_n = d_c.contiguous(), d_n.contiguous()
    M = int(d_n.shape[0])
    if d_c.dtype != torch.int32 or d_n.dtype != torch.int32 or tuple(d_c.shape) != (M, M):
        raise ValueError("common int32 [M, M] and n_contacts int32 [M]")
    q = _lib.PoseClusterRequest()
    q.common, q.n_contacts, q.cutoff_fcc, q.cutoff_reverse = d_c.data_ptr(), d_n.data_ptr(), float(cutoff_fcc), float(cutoff_reverse)
    return _cluster_launch(api, api.pose_cluster, q, d_n, min_size)


def cluster_poses(poses_or_contacts, cutoff_fcc=0.6, strictness=0.75, min_size=4, **contact_options):
    """FCC clustering of docking poses on the device (Rodrigues et al. 2012: the rule of HADDOCK's ``cluster_fcc``, with
    the tie between equally connected centres broken towards the smaller index; tests/fcc_ref.py states it in numpy).
    ``fcc[i, j]`` is the fraction of pose i's interface contacts that pose j has too.  Pose j is a neighbour of i when
    ``fcc[i, j] >= cutoff_fcc`` and ``fcc[j, i] >= cutoff_fcc * strictness``.  The alive pose with the most alive
    neighbours (the smallest index on a tie) becomes a centre as long as it has ``min_size - 1`` of them; it and they
    form a cluster and die.  ``poses_or_contacts``: a ``PoseContacts``, or what ``pose_contacts`` takes together with its
    options (cutoff, heavy_only, table, device, api, chunk).  Returns a ``PoseClusters``.  More poses than
    drgnn_fcc_capacity(2) (4096) are refused (DrgnnError, capacity)."""
    for name, v in (("cutoff_fcc", cutoff_fcc), ("strictness", strictness)):
        if not (float(v) > 0.0 and float(v) <= 1.0):
            raise ValueError("%s must lie in (0, 1]" % name)
    _check_min_size(min_size)
    c = poses_or_contacts
    if isinstance(c, PoseContacts):
        if contact_options:
            raise ValueError("contact options %s come with poses, not with PoseContacts" % sorted(contact_options))
    else:
        c = pose_contacts(c, **contact_options)
    M = len(c)
    if M == 0:
        return _pose_clusters(None, c.n_contacts)
    if M > c.api.fcc_capacity(2):
        _lib._check(-2, "drgnn_pose_cluster")
    count = torch.from_numpy(c.n_contacts.astype(np.int32)).to(c.bits.device)
    r = pose_cluster_raw(c.api, _common_device(c), count, float(cutoff_fcc), float(cutoff_fcc) * float(strictness),
                         int(min_size), c.device)
    return _pose_clusters(r, c.n_contacts)


# ---- contact consensus of poses (csrc/drgnn_consensus.h) ------------------------------------------------------------
def _i32(a, dev):
    """(host int32 array, the same on ``dev``)"""
    host = np.ascontiguousarray(a, dtype=np.int32).reshape(-1)
    return host, torch.from_numpy(host).to(dev)


def _contact_words(bits, n_b):
    """(the contiguous tensor, M, nA) of contact words int64 [M, nA, ceil(n_b / 64)]"""
    if bits.dtype != torch.int64 or bits.dim() != 3 or int(bits.shape[2]) != (int(n_b) + 63) // 64:
        raise ValueError("bits int64 [M, nA, %d]" % ((int(n_b) + 63) // 64))
    return bits.contiguous(), int(bits.shape[0]), int(bits.shape[1])


def contact_counts_raw(api, bits, n_b, order, group_ptr):
    """One drgnn_pose_contact_counts call (include/drgnn.h): ``bits`` a tensor of words int64 [M, nA, WB], ``order`` int
    [L] and ``group_ptr`` int [G+1] numpy arrays.  Returns (counts int32 [G, nA, n_b], residues int32 [G, nA + n_b]) as
    tensors on the device of ``bits``."""
    bits, M, nA = _contact_words(bits, n_b)
    if api is _lib._API:
        _lib.require_device(bits)
    h_order, d_order = _i32(order, bits.device)
    h_ptr, d_ptr = _i32(group_ptr, bits.device)
    G = max(len(h_ptr) - 1, 0)
    counts = torch.empty((G, nA, int(n_b)), dtype=torch.int32, device=bits.device)
    residues = torch.empty((G, nA + int(n_b)), dtype=torch.int32, device=bits.device)
    q = _lib.ContactCountsRequest()
    q.bits, q.order, q.group_ptr = bits.data_ptr(), d_order.data_ptr(), d_ptr.data_ptr()
    q.host_order, q.host_group_ptr = h_order.ctypes.data, h_ptr.ctypes.data
    q.n_poses, q.n_chain_a, q.n_chain_b, q.n_groups, q.n_listed = M, nA, int(n_b), G, len(h_order)
    q.counts, q.residues = counts.data_ptr(), residues.data_ptr()
    api.pose_contact_counts(q, _lib.current_stream(bits))
    return counts, residues


def consensus_numerators_raw(api, bits, n_b, counts, row):
    """One drgnn_pose_consensus_numerators call: ``bits`` words int64 [M, nA, WB] and ``counts`` int32 [G, nA, n_b] as
    tensors on one device, ``row`` int [M] a numpy array (-1: no row).  Returns int64 [M] on that device."""
    bits, M, nA = _contact_words(bits, n_b)
    if counts.dtype != torch.int32 or counts.dim() != 3 or tuple(counts.shape[1:]) != (nA, int(n_b)) or counts.device != bits.device:
        raise ValueError("counts int32 [G, %d, %d] on the device of bits" % (nA, int(n_b)))
    if api is _lib._API:
        _lib.require_device(bits)
    counts = counts.contiguous()
    h_row, d_row = _i32(row, bits.device)
    if len(h_row) != M:
        raise ValueError("%d rows for %d poses" % (len(h_row), M))
    out = torch.empty(M, dtype=torch.int64, device=bits.device)
    q = _lib.ConsensusNumeratorsRequest()
    q.bits, q.counts, q.row, q.host_row = bits.data_ptr(), counts.data_ptr(), d_row.data_ptr(), h_row.ctypes.data
    q.n_poses, q.n_chain_a, q.n_chain_b, q.n_groups, q.numerators = M, nA, int(n_b), int(counts.shape[0]), out.data_ptr()
    api.pose_consensus_numerators(q, _lib.current_stream(bits))
    return out


def consensus_bits_raw(api, counts, min_count):
    """One drgnn_pose_consensus_bits call: ``counts`` int32 [G, nA, nB] a tensor, ``min_count`` int [G] a numpy array.
    Returns (bits int64 [G, nA, WB], n_contacts int32 [G]) as tensors on the device of ``counts``."""
    if counts.dtype != torch.int32 or counts.dim() != 3:
        raise ValueError("counts int32 [G, nA, nB]")
    if api is _lib._API:
        _lib.require_device(counts)
    counts = counts.contiguous()
    G, nA, nB = (int(v) for v in counts.shape)
    h_min, d_min = _i32(min_count, counts.device)
    if len(h_min) != G:
        raise ValueError("%d thresholds for %d groups" % (len(h_min), G))
    bits = torch.empty((G, nA, (nB + 63) // 64), dtype=torch.int64, device=counts.device)
    n = torch.empty(G, dtype=torch.int32, device=counts.device)
    q = _lib.ConsensusBitsRequest()
    q.counts, q.min_count, q.host_min_count = counts.data_ptr(), d_min.data_ptr(), h_min.ctypes.data
    q.n_chain_a, q.n_chain_b, q.n_groups, q.bits, q.n_contacts = nA, nB, G, bits.data_ptr(), n.data_ptr()
    api.pose_consensus_bits(q, _lib.current_stream(counts))
    return bits, n


def _group_rows(groups, M, G, what="groups"):
    """int64 [M] from ``groups`` (None: all 0), checked against [-1, G)"""
    if groups is None:
        g = np.zeros(M, dtype=np.int64)
    else:
        if torch.is_tensor(groups):
            groups = groups.detach().cpu().numpy()
        g = np.asarray(groups)
        if g.ndim != 1 or g.shape[0] != M:
            raise ValueError("%d %s for %d poses" % (g.shape[0] if g.ndim == 1 else g.size, what, M))
        if g.size and not np.issubdtype(g.dtype, np.integer):
            raise ValueError("%s must be integers" % what)
        g = g.astype(np.int64)
    if g.size and (g.min() < -1 or g.max() >= G):
        raise ValueError("%s must lie in [-1, %d)" % (what, G))
    return g


class ContactFrequency(object):
    """``contact_frequency``: ``counts`` int32 [G, nA, nB] (the poses of group g that have residue a of the first chain
    and residue b of the second in contact) and ``residues`` int32 [G, nA + nB] (the poses of g in which a residue has any
    contact) on the device, ``n_poses`` int64 [G] on the host; ``table``, ``n_a`` / ``n_b``, ``cutoff`` and
    ``heavy_only`` of the ``PoseContacts`` it was counted from.  The accessors copy to the host once."""

    def __init__(self, contacts, counts, residues, n_poses):
        self.counts, self.residues, self.n_poses = counts, residues, n_poses
        self.table, self.api, self.device = contacts.table, contacts.api, contacts.device
        self.cutoff, self.heavy_only, self.n_a, self.n_b = contacts.cutoff, contacts.heavy_only, contacts.n_a, contacts.n_b
        self._host = {}

    def __len__(self):
        return int(self.n_poses.shape[0])

    def _on_host(self, name, g):
        if not 0 <= int(g) < len(self):
            raise ValueError("group must lie in [0, %d)" % len(self))
        if name not in self._host:
            self._host[name] = getattr(self, name).cpu().numpy()
        return self._host[name][int(g)]

    def _fraction(self, name, g):
        c, n = self._on_host(name, g).astype(np.float64), self.n_poses[int(g)]
        return c / np.float64(n) if n > 0 else np.zeros_like(c)

    def fraction(self, g=0):
        """float64 [nA, nB]: the fraction of the poses of group g with each contact (zeros for a group without poses)"""
        return self._fraction("counts", g)

    def residue_fraction(self, g=0):
        """float64 [R]: the fraction of the poses of group g in which each residue of the table is in contact: a
        per-residue array for ``attach_residue_features``"""
        return self._fraction("residues", g)

    def pairs(self, g=0, min_count=1):
        """int32 [n, 3]: (residue of the first chain, residue of the second, count) of the contacts at least
        ``min_count`` poses of group g have, both indices into the table's residues, sorted by the pair"""
        if int(min_count) != min_count or int(min_count) < 1:
            raise ValueError("min_count must be an integer >= 1")
        c = self._on_host("counts", g)
        a, b = np.nonzero(c >= int(min_count))
        return np.stack((a, b + self.n_a, c[a, b]), axis=1).astype(np.int32)

    def interface_residues(self, g=0, min_poses=1):
        """int64 [n], sorted: the residues in contact in at least ``min_poses`` poses of group g (for one group of all
        poses: ``interface_residues(contacts, min_poses)``)"""
        if int(min_poses) != min_poses or int(min_poses) < 1:
            raise ValueError("min_poses must be an integer >= 1")
        return np.flatnonzero(self._on_host("residues", g) >= int(min_poses)).astype(np.int64)


def contact_frequency(contacts, groups=None, n_groups=None):
    """How often the poses of a ``PoseContacts``, or of every group of them, have each residue pair in contact: the
    consensus map of CONSRANK (Oliva, Vangone and Cavallo 2013; tests/consensus_ref.py states the rule), counted on the
    device in one launch, linear in the poses.  ``groups`` int [M]: the group of every pose, -1 for none
    (``PoseClusters.labels`` as it is); None: one group of all poses.  ``n_groups``: G (default: the largest group + 1).
    A group lists its poses in index order.  Returns a ``ContactFrequency``."""
    if not isinstance(contacts, PoseContacts):
        raise ValueError("a contact frequency is taken from PoseContacts (pose_contacts)")
    M = len(contacts)
    if n_groups is not None and (int(n_groups) != n_groups or int(n_groups) < 0):
        raise ValueError("n_groups must be an integer >= 0")
    if groups is None:
        G = 1 if n_groups is None else int(n_groups)
        g = _group_rows(None, M, max(G, 1)) if G > 0 else np.full(M, -1, dtype=np.int64)
    else:
        g = _group_rows(groups, M, np.iinfo(np.int32).max if n_groups is None else int(n_groups))
        G = int(n_groups) if n_groups is not None else int(g.max()) + 1 if g.size else 0
    order = np.argsort(g, kind="stable")
    order = order[g[order] >= 0]
    group_ptr = np.concatenate(([0], np.cumsum(np.bincount(g[order], minlength=G)))).astype(np.int64)
    counts, residues = contact_counts_raw(contacts.api, contacts.bits, contacts.n_b, order, group_ptr)
    return ContactFrequency(contacts, counts, residues, np.diff(group_ptr).astype(np.int64))


def consensus_scores(contacts, frequency=None, groups=None, leave_one_out=False, return_numerators=False):
    """float64 [M]: the CONSRANK score of every pose of a ``PoseContacts``, the mean frequency of its contacts:
    ``num / (n * N)`` with num the sum of ``counts[row]`` over the pose's n contacts and N the poses of its row, one
    float64 division on the integers; 0.0 for a pose without contacts or in no group.  Without ``frequency`` the one of
    ``contacts`` and ``groups`` is built and every pose is scored against its own group; ``leave_one_out`` then leaves
    the pose itself out of its frequency, ``(num - n) / (n * (N - 1))`` (0.0 in a group of one).  With a ``frequency``
    any ``PoseContacts`` of its topology, library and device is scored, ``groups`` naming the row of every pose (None:
    row 0).  ``return_numerators``: (scores, num int64 [M])."""
    if not isinstance(contacts, PoseContacts):
        raise ValueError("consensus scores are taken of PoseContacts (pose_contacts)")
    M = len(contacts)
    if frequency is None:
        frequency = contact_frequency(contacts, groups)
        row = _group_rows(groups, M, max(len(frequency), 1))
    else:
        if leave_one_out:
            raise ValueError("leave_one_out needs the frequency built in the same call: a given frequency may not list the pose once")
        f = frequency
        if not isinstance(f, ContactFrequency):
            raise ValueError("frequency is a ContactFrequency (contact_frequency)")
        if (contacts.n_a, contacts.n_b) != (f.n_a, f.n_b) or contacts.api is not f.api or torch.device(contacts.device) != torch.device(f.device):
            raise ValueError("the contacts and the frequency must be of one topology, library and device")
        row = _group_rows(groups, M, len(f))
    api, step = contacts.api, max(1, contacts.api.consensus_capacity(3))
    parts = [consensus_numerators_raw(api, contacts.bits[lo:lo + step], contacts.n_b, frequency.counts, row[lo:lo + step])
             for lo in range(0, M, step)]
    num = np.concatenate([p.cpu().numpy() for p in parts]).astype(np.int64) if parts else np.zeros(0, np.int64)
    n = contacts.n_contacts.astype(np.int64)
    N = np.where(row >= 0, frequency.n_poses[np.maximum(row, 0)] if len(frequency) else 0, 0).astype(np.int64)
    top, den = (num - n, n * (N - 1)) if leave_one_out else (num, n * N)
    scores = np.zeros(M, dtype=np.float64)
    has = den > 0
    scores[has] = top[has].astype(np.float64) / den[has].astype(np.float64)
    return (scores, num) if return_numerators else scores


def consensus_contacts(frequency, min_fraction=0.5, min_count=None):
    """The consensus map of every group of a ``ContactFrequency`` as a ``PoseContacts`` of G rows: contact (a, b) of row g
    is set when at least ``min_count`` poses of g have it; ``min_fraction`` in (0, 1] means ``max(1, ceil(min_fraction *
    N_g))`` (float64), ``min_count`` an integer >= 1 (or one per group) instead.  ``fcc_matrix(poses, consensus)``,
    ``common_contacts``, ``interface_residues`` and ``pose_rmsd(kind="interface", residues=...)`` take it like any
    pose."""
    if not isinstance(frequency, ContactFrequency):
        raise ValueError("consensus contacts are taken from a ContactFrequency (contact_frequency)")
    G = len(frequency)
    if min_count is None:
        if not (float(min_fraction) > 0.0 and float(min_fraction) <= 1.0):
            raise ValueError("min_fraction must lie in (0, 1]")
        least = np.array([max(1, int(np.ceil(np.float64(min_fraction) * np.float64(n)))) for n in frequency.n_poses], dtype=np.int64)
    else:
        least = np.asarray(min_count)
        if (least.size and not np.issubdtype(least.dtype, np.integer)) or least.shape not in ((), (G,)) or (least < 1).any():
            raise ValueError("min_count must be an integer >= 1, or one per group")
        least = np.broadcast_to(least, (G,)).astype(np.int64)
    bits, n = consensus_bits_raw(frequency.api, frequency.counts, least)
    return PoseContacts(frequency.table, bits, n.cpu().numpy().astype(np.int64), frequency.api, frequency.device,
                        frequency.cutoff, frequency.heavy_only)


# ---- pairwise pose RMSD and RMSD clustering of poses (csrc/drgnn_rmsd.h) --------------------------------------------
RMSD_KINDS = ("ligand", "interface", "fixed", "all")
RMSD_WORKSPACE_BUDGET = 1 << 30    # bytes of fp64 pose records one drgnn_pose_rmsd call may ask for (sets the default chunk)


def select_atoms(table, names=BACKBONE, chain=None, residues=None):
    """int32 [n]: the atoms of ``table``, in its grouped atom order, whose name is one of ``names`` (None: every name;
    names need a table built with ``atom_name=``), that belong to ``chain`` (0 or 1, None: both) and to one of
    ``residues`` (indices into the table's residues, None: all)."""
    keep = np.ones(table.n_atoms, dtype=bool)
    if names is not None:
        if table.atom_name is None:
            raise ValueError("atoms are selected by name: build the AtomTable with atom_name=")
        keep &= np.isin(table.atom_name, list(names))
    res_of_atom = np.repeat(np.arange(table.n_residues), np.diff(table.atom_ptr))
    if chain is not None:
        if chain not in (0, 1):
            raise ValueError("chain must be 0, 1 or None")
        keep &= table.res_chain[res_of_atom] == chain
    if residues is not None:
        r = np.asarray(residues, dtype=np.int64).reshape(-1)
        if r.size and (r.min() < 0 or r.max() >= table.n_residues):
            raise ValueError("residues must be indices into the table's %d residues" % table.n_residues)
        on = np.zeros(table.n_residues, dtype=bool)
        on[r] = True
        keep &= on[res_of_atom]
    return np.flatnonzero(keep).astype(np.int32)


def _atom_list(what, idx, n_atoms, least):
    a = np.asarray(idx)
    if a.ndim != 1 or (a.size and a.dtype.kind not in "iu"):
        raise ValueError("%s must be a list of atom indices" % what)
    if a.size < least:
        raise ValueError("%s needs at least %d atom%s" % (what, least, "" if least == 1 else "s"))
    if a.min() < 0 or a.max() >= n_atoms:
        raise ValueError("%s must be indices into the table's %d atoms" % (what, n_atoms))
    return np.ascontiguousarray(a, dtype=np.int32)


def rmsd_selection(table, rms=None, fit=None, kind=None, residues=None):
    """(rms int32 [nR], fit int32 [nF] or None) of ``pose_rmsd``: the two lists as given, or what ``kind`` stands for"""
    if kind is None:
        if rms is None:
            raise ValueError("pose_rmsd needs rms= (atom indices) or kind= (one of %s)" % ", ".join(RMSD_KINDS))
        if residues is not None:
            raise ValueError("residues= goes with kind=\"interface\"")
        return _atom_list("rms", rms, table.n_atoms, 1), None if fit is None else _atom_list("fit", fit, table.n_atoms, 3)
    if kind not in RMSD_KINDS:
        raise ValueError("kind must be one of %s" % ", ".join(RMSD_KINDS))
    if rms is not None or fit is not None:
        raise ValueError("kind= stands for rms= and fit=: give one or the other")
    if (kind == "interface") != (residues is not None):
        raise ValueError("residues= goes with kind=\"interface\", and that kind needs it")
    long_chain = 0 if table.split >= table.n_residues - table.split else 1
    if kind == "ligand":
        rms, fit = select_atoms(table, chain=1 - long_chain), select_atoms(table, chain=long_chain)
    elif kind == "fixed":
        rms, fit = select_atoms(table, chain=1 - long_chain), None
    else:
        rms = fit = select_atoms(table, residues=residues)
    return _atom_list("the rms atoms of kind %r" % kind, rms, table.n_atoms, 1), \
        None if fit is None else _atom_list("the fit atoms of kind %r" % kind, fit, table.n_atoms, 3)


def pose_rmsd_raw(api, xyz_a, xyz_b, rms_idx, fit_idx=None, phases=0, workspace=None, out=None):
    """One drgnn_pose_rmsd call (include/drgnn.h): ``xyz_a`` / ``xyz_b`` float32 tensors [Ma, T, 3] / [Mb, T, 3] on one
    device (the same tensor: the square matrix of one batch), the lists as numpy int32.  Returns float64 [Ma, Mb] on
    that device.  ``workspace`` / ``out``: tensors kept between calls that run the launches one by one (``phases``)."""
    rms_host = np.ascontiguousarray(rms_idx, dtype=np.int32)
    fit_host = None if fit_idx is None else np.ascontiguousarray(fit_idx, dtype=np.int32)
    xyz_a, xyz_b = xyz_a.contiguous(), xyz_b.contiguous()
    if xyz_a.dtype != torch.float32 or xyz_b.dtype != torch.float32 or xyz_a.dim() != 3 or xyz_b.dim() != 3 or \
            xyz_a.shape[1:] != xyz_b.shape[1:] or xyz_a.shape[2] != 3:
        raise ValueError("xyz float32 [Ma, T, 3] and [Mb, T, 3]")
    if api is _lib._API:
        _lib.require_device(xyz_a)
    dev = xyz_a.device
    Ma, Mb, nF = int(xyz_a.shape[0]), int(xyz_b.shape[0]), 0 if fit_host is None else len(fit_host)
    d_rms = torch.from_numpy(rms_host).to(dev)
    d_fit = None if fit_host is None else torch.from_numpy(fit_host).to(dev)
    nbytes = api.rmsd_workspace(Ma, Mb, nF, len(rms_host))[0]
    if workspace is None:
        workspace = torch.empty(max(nbytes // 8, 1), dtype=torch.float64, device=dev)
    d = torch.empty((Ma, Mb), dtype=torch.float64, device=dev) if out is None else out
    q = _lib.PoseRmsdRequest()
    q.xyz_a, q.xyz_b = xyz_a.data_ptr() if Ma else None, xyz_b.data_ptr() if Mb else None
    q.rms_idx, q.host_rms_idx = d_rms.data_ptr() if len(rms_host) else None, rms_host.ctypes.data if len(rms_host) else None
    if nF:
        q.fit_idx, q.host_fit_idx = d_fit.data_ptr(), fit_host.ctypes.data
    q.n_a, q.n_b, q.n_atoms, q.n_fit, q.n_rms, q.phases = Ma, Mb, int(xyz_a.shape[1]), nF, len(rms_host), int(phases)
    q.workspace, q.workspace_bytes, q.d = workspace.data_ptr(), workspace.numel() * 8, d.data_ptr() if Ma and Mb else None
    api.pose_rmsd(q, _lib.current_stream(xyz_a))
    return d


def pose_rmsd(poses, rms=None, fit=None, kind=None, other=None, residues=None, device=None, api=None, chunk=None, table=None):
    """The pose-by-pose RMSD matrix of M poses of one topology (an ``AtomTable.poses`` batch, a table, or xyz float32
    [M,T,3] in the grouped atom order of ``table``), on the device: a float64 tensor [M, M], or [M, M'] against the poses
    ``other`` of the same table.  ``rms``: the atoms the RMSD is taken over (indices in the table's grouped order, as
    ``select_atoms`` returns them); ``fit``: the atoms (at least 3, not collinear) that pose i is superposed on pose j
    by, with the optimal proper rotation and translation, before the RMSD is taken; None: no superposition.  ``kind``
    stands for both: ``"ligand"`` fit on the backbone of the chain with more residues (the first on a tie), RMSD of the
    other chain's backbone (pairwise l-RMSD); ``"interface"`` fit = rms = the backbone of ``residues`` (``interface_residues``;
    pairwise i-RMSD); ``"fixed"`` no superposition, the shorter chain's backbone (rigid-body runs with a fixed receptor);
    ``"all"`` fit = rms = every backbone atom.  tests/rmsd_ref.py states the rule.  The matrix is exactly symmetric with
    a zero diagonal; an entry does not depend on M, on ``chunk`` (poses per side of one launch, at most
    drgnn_rmsd_capacity(0)), on the side or the place of its poses or on the run."""
    t, xyz = _pose_batch(poses, table)
    xyz2 = None
    if other is not None:
        xyz2 = _pose_batch(other, t, "the other poses must be of the same AtomTable")[1]
    rms_idx, fit_idx = rmsd_selection(t, rms, fit, kind, residues)
    api = api or _lib.get()
    device = _default_device(api, device)
    dev = torch.device(device)
    # only the selected atoms are uploaded
    cols = np.unique(np.concatenate((rms_idx, fit_idx if fit_idx is not None else rms_idx[:0])))
    rms_idx = np.searchsorted(cols, rms_idx).astype(np.int32)
    fit_idx = None if fit_idx is None else np.searchsorted(cols, fit_idx).astype(np.int32)
    record = 8 * (3 * (len(rms_idx) + (0 if fit_idx is None else len(fit_idx))) + 2)
    cap = min(api.rmsd_capacity(0), max(1, RMSD_WORKSPACE_BUDGET // (2 * record)))
    chunk = cap if chunk is None else max(1, min(int(chunk), cap))
    M, M2 = int(xyz.shape[0]), int(xyz.shape[0] if xyz2 is None else xyz2.shape[0])
    if M == 0 or M2 == 0:
        return torch.zeros((M, M2), dtype=torch.float64, device=dev)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x[:, cols], dtype=np.float32)).to(dev)
    A = up(xyz)
    B = A if xyz2 is None else up(xyz2)
    return _blocked_pairs(lambda x, y: pose_rmsd_raw(api, x, y, rms_idx, fit_idx), A, B, chunk, torch.float64, xyz2 is None)


def interface_residues(contacts, min_poses=1):
    """int64 [n], sorted: the residues (indices into the table's residues, both chains) that are in contact in at least
    ``min_poses`` poses of a ``PoseContacts``: what ``pose_rmsd(kind="interface", residues=...)`` takes"""
    if not isinstance(contacts, PoseContacts):
        raise ValueError("interface residues are taken from PoseContacts (pose_contacts)")
    if int(min_poses) != min_poses or int(min_poses) < 1:
        raise ValueError("min_poses must be an integer >= 1")
    w = contacts.words()                                               # uint64 [M, nA, WB]
    if w.size == 0:
        return np.zeros(0, np.int64)
    in_a = (w != 0).any(axis=2).sum(axis=0)                            # poses in which a row has a bit
    cols = np.bitwise_or.reduce(w, axis=1)                             # [M, WB]: the OR over the rows
    in_b = np.unpackbits(np.ascontiguousarray(cols).view(np.uint8), axis=1, bitorder="little")[:, :contacts.n_b].sum(axis=0)
    return np.concatenate((np.flatnonzero(in_a >= int(min_poses)), contacts.n_a + np.flatnonzero(in_b >= int(min_poses)))).astype(np.int64)


def pose_cluster_dist_raw(api, d, cutoff=7.5, min_size=4, device="cpu"):
    """One drgnn_pose_cluster_dist call (include/drgnn.h): ``d`` float64 [M, M] as a numpy array or a tensor on
    ``device``.  Returns what ``pose_cluster_raw`` returns."""
    dev = torch.device(device)
    d_d = (d if torch.is_tensor(d) else torch.from_numpy(np.ascontiguousarray(d, dtype=np.float64)).to(dev)).contiguous()
    M = int(d_d.shape[0])
    if d_d.dtype != torch.float64 or tuple(d_d.shape) != (M, M):
        raise ValueError("d float64 [M, M]")
    q = _lib.PoseClusterDistRequest()
    q.d, q.cutoff = d_d.data_ptr(), float(cutoff)
    return _cluster_launch(api, api.pose_cluster_dist, q, d_d, min_size)


def cluster_poses_rmsd(poses_or_matrix, cutoff=7.5, min_size=4, **rmsd_options):
    """RMSD clustering of docking poses on the device (the rule of HADDOCK's ``cluster_struc`` and of ClusPro, with the
    tie between equally connected centres broken towards the smaller index; tests/rmsd_ref.py states it in numpy).  Pose
    j is a neighbour of i when ``D[i, j] <= cutoff`` (A).  The alive pose with the most alive neighbours (the smallest
    index on a tie) becomes a centre as long as it has ``min_size - 1`` of them; it and they form a cluster and die.
    ``poses_or_matrix``: a square float64 matrix (a tensor, as ``pose_rmsd`` returns it, or a numpy array; ``api`` and
    ``device`` are then the only options), or what ``pose_rmsd`` takes together with its options (rms, fit, kind,
    residues, table, device, api, chunk).  Returns a ``PoseClusters`` with ``n_contacts`` None.  More poses than
    drgnn_rmsd_capacity(1) (4096) are refused (DrgnnError, capacity)."""
    if not (float(cutoff) > 0.0 and float(cutoff) < float("inf")):
        raise ValueError("cutoff must be a positive finite number")
    _check_min_size(min_size)
    if "other" in rmsd_options:
        raise ValueError("clustering takes the square matrix of one batch: no other=")
    p = poses_or_matrix
    is_matrix = (torch.is_tensor(p) or isinstance(p, np.ndarray)) and p.ndim == 2
    api = rmsd_options.get("api") or _lib.get()
    device = _default_device(api, rmsd_options.get("device") or (str(p.device) if torch.is_tensor(p) and is_matrix else None))
    if is_matrix:
        if set(rmsd_options) - {"api", "device"}:
            raise ValueError("rmsd options %s come with poses, not with a matrix" % sorted(set(rmsd_options) - {"api", "device"}))
        if p.shape[0] != p.shape[1]:
            raise ValueError("a distance matrix is square")
        M = int(p.shape[0])
    else:
        M = len(p) if isinstance(p, Poses) else 1 if isinstance(p, AtomTable) else int(np.asarray(p).shape[0])
    if M > api.rmsd_capacity(1):
        _lib._check(-2, "drgnn_pose_cluster_dist")
    if M == 0:
        if not is_matrix:
            pose_rmsd(p, **dict(rmsd_options, api=api, device=device))             # (the options are checked; nothing is launched)
        return _pose_clusters(None, None)
    d = p if is_matrix else pose_rmsd(p, **dict(rmsd_options, api=api, device=device))
    if torch.is_tensor(d):
        d = d.to(torch.float64)
    r = pose_cluster_dist_raw(api, d, float(cutoff), int(min_size), device)
    return _pose_clusters(r, None)
