"""MI355X-native message-passing hot path of Deeprank-GNN (GINet / sGAT / FoutNet
convolutions + community pooling), behind the reference's own model API.

Importing the package never touches the GPU or the HIP library; the first call that
needs a kernel loads ``csrc/libdrgnn.so`` and raises if it (or a GPU) is missing --
there is no CPU fallback in the product path.
"""
from .data import Batch, Data, DataLoader  # noqa: F401
from .ginet import GINet  # noqa: F401
from .sGAT import sGAT  # noqa: F401
from .foutnet import FoutNet  # noqa: F401
from .metrics import Metrics  # noqa: F401
from .ensemble import Ensemble  # noqa: F401
from .cohort import Cohort, kfold_indices  # noqa: F401
from .interface import (AtomTable, LddtReference, ScoreReference, attach_residue_features, attach_scores, bsa_radii,  # noqa: F401
                        cluster_poses, cluster_poses_rmsd, common_contacts, consensus_contacts, consensus_scores,
                        contact_frequency, depth_radii, docking_scores, fcc_matrix, hse_table,
                        interface_graphs, interface_residues, interface_resident_set, lddt_scores, pose_contacts, pose_rmsd,
                        read_pdb_atom_names, read_pdb_atoms, residue_bsa, residue_depth, residue_hse, select_atoms)

__version__ = "0.1.0"
