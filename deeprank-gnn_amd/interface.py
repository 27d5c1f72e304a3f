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

and the superposition-free lDDT of the poses (Mariani et al. 2013; csrc/drgnn_lddt.h), over all atom pairs, over the
inter-chain ones (the interface lDDT) and per residue:

    lref = LddtReference(table, rc, rs, rn, rx)                # once per complex, on the host
    q = lddt_scores(poses, lref, per_residue=True)             # lddt, ilddt [M], residue_lddt [M, R]
    store = interface_graphs(poses, names, lddt=lref)          # score/lddt, score/ilddt and node_data/lddt

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

from .atoms import (  # noqa: F401
    AtomTable, BACKBONE, Poses, RESIDUE_CHARGE, RESIDUE_NAMES, RESIDUE_POLARITY, _TYPE_OF, _complexes,
    _default_device, _pose_batch, _ragged, counted_atoms, read_pdb_atom_names, read_pdb_atoms, select_atoms)
from .residue_features import (  # noqa: F401
    BSA, BSA_BACKBONE, BSA_FIRST_LETTER, BSA_SIDE_CHAIN, BSA_XYZ_BUDGET, DEPTH, DEPTH_COMPONENTS, DEPTH_OTHER,
    DEPTH_UNITED, DEPTH_WORKSPACE_BUDGET, FEATURES, Feature, HSE, HSE_BACKBONE, HSE_CONNECT, HSE_DIRECTION, HSE_TILE,
    HSE_WORKGROUPS, RESIDUE_XYZ_BUDGET, _C, _CR, _CT, _N, _O1, _O2, _S, _bsa_graph_options, _bsa_options,
    _depth_graph_options, _depth_options, _depth_too_large, _feature_chunk, _hse_graph_options, _hse_node_data,
    _hse_options, _per_table, _residue_values, _targets, bsa_radii, bsa_raw, depth_dots, depth_link, depth_radii,
    depth_raw, hse_raw, hse_table, hse_tile, residue_bsa, residue_depth, residue_hse)
from .dock_scores import (  # noqa: F401
    LDDT_KEYS, LDDT_THRESHOLDS, LddtReference, SCORE_KEYS, SCORE_XYZ_BUDGET, ScoreReference, _heavy, _residue_pairs,
    attach_scores, dock_scores_raw, docking_scores, lddt_raw, lddt_scores)
from .iface_graphs import (  # noqa: F401
    FEATURE_WIDTH, MCL_WORKSPACE_BUDGET, PACK_SOURCE, WORKSPACE_BUDGET, _mcl_groups, _pack_columns, _residue_tables,
    attach_residue_features, build_ragged, build_ragged_device, default_chunk, iface_pack_raw, interface_graphs,
    interface_resident_set, pack_request, pack_type_table)
from .poses import (  # noqa: F401
    ContactFrequency, FCC_XYZ_BUDGET, PoseClusters, PoseContacts, RMSD_KINDS, RMSD_WORKSPACE_BUDGET, _atom_list,
    _blocked_pairs, _check_min_size, _cluster_launch, _common_device, _contact_words, _group_rows, _pose_clusters,
    cluster_poses, cluster_poses_rmsd, common_contacts, consensus_bits_raw, consensus_contacts,
    consensus_numerators_raw, consensus_scores, contact_counts_raw, contact_frequency, fcc_matrix, interface_residues,
    pose_cluster_dist_raw, pose_cluster_raw, pose_common_raw, pose_contacts, pose_contacts_raw, pose_rmsd,
    pose_rmsd_raw, rmsd_selection)
