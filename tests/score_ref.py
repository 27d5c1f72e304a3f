"""The docking scores in numpy float64, written for the tests: Kabsch by SVD with the determinant correction, every
atom transformed explicitly, brute-force contacts over all atom pairs.  It shares no code with the package (whose
kernel goes through moments and Horn's quaternion matrix): atoms are plain per-atom arrays in any order, matched through
a dictionary.

Rules (include/drgnn.h, the scores section): atoms correspond when (chain, res_seq, atom name) are equal; backbone = CA,
C, N, O; a residue pair exists when an atom pair lies at d <= cutoff; fnat over the reference's pairs at 5.0 A; the
interface zone = the residues of the reference's pairs at 10.0 A; the long chain has more residues in the reference
(chain A on a tie)."""
import numpy as np

BACKBONE = ("CA", "C", "N", "O")


def contacts(chain, seq, xyz, cutoff, chains=("A", "B")):
    """{(res_seq of A, res_seq of B)} with an atom pair at d <= cutoff"""
    chain, seq, xyz = np.asarray(chain), np.asarray(seq), np.asarray(xyz, dtype=np.float64)
    ia, ib = np.flatnonzero(chain == chains[0]), np.flatnonzero(chain == chains[1])
    d2 = np.zeros((len(ia), len(ib)))
    for k in range(3):
        d2 += (xyz[ia, k][:, None] - xyz[ib, k][None, :]) ** 2
    p, q = np.nonzero(np.sqrt(d2) <= cutoff)
    return set(zip(seq[ia][p].tolist(), seq[ib][q].tolist()))


def kabsch(P, Q):
    """(R, centroid of P, centroid of Q): the proper rotation with R (p - pc) ~ q - qc in the least-squares sense"""
    pc, qc = P.mean(axis=0), Q.mean(axis=0)
    U, _, Vt = np.linalg.svd((P - pc).T @ (Q - qc))
    d = np.sign(np.linalg.det(Vt.T @ U.T))
    R = Vt.T @ np.diag([1.0, 1.0, d]) @ U.T
    return R, pc, qc


def rmsd_after(R, pc, qc, P, Q):
    return float(np.sqrt((((P - pc) @ R.T - (Q - qc)) ** 2).sum(axis=1).mean()))


def classes(irmsd):
    capri = 5
    for thr, val in zip([6.0, 4.0, 2.0, 1.0], [4, 3, 2, 1]):
        if irmsd < thr:
            capri = val
    return int(irmsd < 4.0), capri


class Reference(object):
    def __init__(self, chain, seq, name, xyz, izone_cutoff=10.0, fnat_cutoff=5.0, chains=("A", "B")):
        self.chains = chains
        self.fnat_cutoff = fnat_cutoff
        chain, seq = np.asarray(chain), np.asarray(seq)
        self.pairs = contacts(chain, seq, xyz, fnat_cutoff, chains)
        near = contacts(chain, seq, xyz, izone_cutoff, chains)
        self.izone = {(chains[0], a) for a, _ in near} | {(chains[1], b) for _, b in near}
        n_res = [len(set(seq[chain == c].tolist())) for c in chains]
        self.long_chain = chains[0] if n_res[0] >= n_res[1] else chains[1]
        self.atoms = {}
        for c, s, n, x in zip(chain.tolist(), seq.tolist(), np.asarray(name).tolist(), np.asarray(xyz, dtype=np.float64)):
            if c in chains:
                self.atoms.setdefault((c, s, n), x)

    def zones(self, chain, seq, name):
        """[keys of the interface zone, of the long chain, of the short chain]: matched backbone atoms"""
        seen, keys = set(), []
        for k in zip(np.asarray(chain).tolist(), np.asarray(seq).tolist(), np.asarray(name).tolist()):
            if k[2] in BACKBONE and k in self.atoms and k not in seen:
                seen.add(k)
                keys.append(k)
        return ([k for k in keys if (k[0], k[1]) in self.izone], [k for k in keys if k[0] == self.long_chain],
                [k for k in keys if k[0] != self.long_chain])

    def score(self, chain, seq, name, xyz):
        """the scores of one decoy given per atom; xyz as the kernel sees it (float32 values) in float64"""
        xyz = np.asarray(xyz, dtype=np.float64)
        dec = {}
        for k, x in zip(zip(np.asarray(chain).tolist(), np.asarray(seq).tolist(), np.asarray(name).tolist()), xyz):
            dec.setdefault(k, x)
        kept = self.pairs & contacts(chain, seq, xyz, self.fnat_cutoff, self.chains)
        fnat = len(kept) / len(self.pairs)
        zi, zl, zs = self.zones(chain, seq, name)
        P, Q = (lambda ks: (np.array([dec[k] for k in ks]), np.array([self.atoms[k] for k in ks])))(zi)
        irmsd = rmsd_after(*kabsch(P, Q), P, Q)
        Pl, Ql = np.array([dec[k] for k in zl]), np.array([self.atoms[k] for k in zl])
        Ps, Qs = np.array([dec[k] for k in zs]), np.array([self.atoms[k] for k in zs])
        lrmsd = rmsd_after(*kabsch(Pl, Ql), Ps, Qs)
        dockq = (fnat + 1.0 / (1.0 + (irmsd / 1.5) ** 2) + 1.0 / (1.0 + (lrmsd / 8.5) ** 2)) / 3.0
        b, c = classes(irmsd)
        return {"irmsd": irmsd, "lrmsd": lrmsd, "fnat": fnat, "dockQ": dockq, "binclass": b, "capri_class": c,
                "n_preserved": len(kept), "preserved": kept, "n_ref_pairs": len(self.pairs),
                "zone_sizes": (len(zi), len(zl), len(zs))}
