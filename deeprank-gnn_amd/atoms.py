"""The atoms of two-chain complexes as the kernels take them: the residue tables of the reference, the PDB readers,
``AtomTable`` and ``Poses``, the ragged batch of a list of complexes and the atom selections the pose calls share."""
import numpy as np

from . import _lib

# this reference version's tables (ResidueGraph.py:43-60): index = the `type` of the residue
RESIDUE_NAMES = ("CYS", "HIS", "ASN", "GLN", "SER", "THR", "TYR", "TRP", "ALA", "PHE",
                 "GLY", "ILE", "VAL", "MET", "PRO", "LEU", "GLU", "ASP", "LYS", "ARG")
RESIDUE_CHARGE = np.array([-0.64, -0.29, -1.22, -1.22, -0.80, -0.80, -0.80, -0.79, -0.37, -0.37,
                           -0.37, -0.37, -0.37, -0.37, 0.0, -0.37, -1.37, -1.37, -0.36, -1.65])
# 0 apolar, 1 polar, 2 negatively charged, 3 positively charged (LYS is listed as negatively charged there)
RESIDUE_POLARITY = np.array([1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0, 2, 2, 2, 3])
_TYPE_OF = {n: i for i, n in enumerate(RESIDUE_NAMES)}
BACKBONE = ("CA", "C", "N", "O")


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
