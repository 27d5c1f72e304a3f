"""The layer under the interface subsystems: the request filler (deeprank_gnn_amd._request), the invariant of the request
records it relies on, the one place that assigns ``host_*`` fields, the facade ``deeprank_gnn_amd.interface`` keeps over
the modules it was split into, and the table that registers the request entry points on ``_lib.Api``.  CPU only."""
import ast
import ctypes
import gc
import glob
import importlib
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from emu_api import emu

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
PACKAGE = os.path.join(ROOT, "deeprank-gnn_amd")


@pytest.fixture(scope="module")
def api():
    return emu()


# ---- the filler -----------------------------------------------------------------------------------------------------
def test_a_checked_table_is_one_host_copy_and_its_upload():
    from deeprank_gnn_amd import _lib
    from deeprank_gnn_amd._request import Request
    view = np.arange(12)[::2]                                          # strided int64
    r = Request(_lib.BsaRequest, "cpu")
    host, dev = r.table("target_res", view)
    assert host.dtype == np.int32 and host.flags["C_CONTIGUOUS"] and host.shape == (6,)
    assert np.array_equal(host, view) and np.array_equal(dev.numpy(), view)
    assert dev.dtype == torch.int32 and dev.device.type == "cpu"
    assert r.q.target_res == dev.data_ptr() and r.q.host_target_res == host.ctypes.data
    q, ids = r.q, (id(host), id(dev))
    del r, host, dev, view
    gc.collect()
    alive = {id(o) for o in q._held}                                   # the record alone keeps both alive
    assert set(ids) <= alive
    kept_host = [o for o in q._held if isinstance(o, np.ndarray)][0]
    kept_dev = [o for o in q._held if torch.is_tensor(o)][0]
    assert q.host_target_res == kept_host.ctypes.data and q.target_res == kept_dev.data_ptr()
    assert np.array_equal(kept_host, np.arange(12)[::2]) and np.array_equal(kept_dev.numpy(), np.arange(12)[::2])


def test_a_table_keeps_the_shape_and_dtype_asked_for():
    from deeprank_gnn_amd import _lib
    from deeprank_gnn_amd._request import Request
    r = Request(_lib.HseRequest, "cpu")
    host, dev = r.table("bb", np.arange(10, dtype=np.int64), shape=(-1, 5))
    assert host.shape == (2, 5) and tuple(dev.shape) == (2, 5) and host.dtype == np.int32
    r = Request(_lib.ScoreRequest, "cpu")
    host = r.host_table("zone_ptr", [0, 3, 6, 9])                      # the host-only table
    assert host.dtype == np.int32 and r.q.host_zone_ptr == host.ctypes.data and any(o is host for o in r.held)


def test_an_empty_table_or_tensor_is_null_on_both_sides():
    from deeprank_gnn_amd import _lib
    from deeprank_gnn_amd._request import Request
    r = Request(_lib.BsaRequest, "cpu")
    host, dev = r.table("target_res", np.zeros(0, np.int64))
    assert host.size == 0 and dev.numel() == 0 and r.q.target_res is None and r.q.host_target_res is None
    r.input("xyz", np.zeros((0, 3)), torch.float32)
    out = r.output("out", (0, 3), torch.float64)
    assert r.q.xyz is None and r.q.out is None and tuple(out.shape) == (0, 3)


def test_a_device_copy_of_another_length_or_dtype_is_refused():
    from deeprank_gnn_amd import _lib
    from deeprank_gnn_amd._request import Request
    table = np.arange(6, dtype=np.int32)
    good = torch.from_numpy(table.copy())
    r = Request(_lib.ScoreRequest, "cpu")
    assert r.table("zone_atom", table, device_copy=good)[1] is good and r.q.zone_atom == good.data_ptr()
    assert r.q.host_zone_atom == table.ctypes.data
    for bad in (good[:5].clone(), good.to(torch.int64), torch.arange(12, dtype=torch.int32)[::2]):
        with pytest.raises(ValueError, match="device copy of zone_atom"):
            Request(_lib.ScoreRequest, "cpu").table("zone_atom", table, device_copy=bad)


def test_inputs_outputs_and_scalars():
    from deeprank_gnn_amd import _lib
    from deeprank_gnn_amd._request import Request
    r = Request(_lib.PoseClusterRequest, "cpu")
    for shape, dtype, zeros in (((3, 5), torch.float64, False), (7, torch.int32, True), ((2, 2, 2), torch.int64, True)):
        out = r.output("labels", shape, dtype, zeros=zeros)
        assert tuple(out.shape) == (shape if isinstance(shape, tuple) else (shape,)) and out.dtype == dtype
        assert out.device.type == "cpu" and r.q.labels == out.data_ptr() and (not zeros or not out.any())
    rows = r.output(("neighbours", "transposed"), (2, 4, 1), torch.int64, zeros=True)
    assert r.q.neighbours == rows[0].data_ptr() and r.q.transposed == rows[1].data_ptr()
    up = r.input("n_contacts", np.arange(4, dtype=np.int64), torch.int32, (None,), "no")
    assert up.dtype == torch.int32 and r.q.n_contacts == up.data_ptr()
    strided = torch.arange(32, dtype=torch.int32).reshape(4, 8)[:, ::2]
    made = r.input("common", strided, torch.int32, (4, 4), "no")
    assert made.is_contiguous() and torch.equal(made, strided) and r.q.common == made.data_ptr()
    for bad in (strided.to(torch.int64), torch.zeros((4, 5), dtype=torch.int32), torch.zeros(16, dtype=torch.int32)):
        with pytest.raises(ValueError, match="common int32"):
            r.input("common", bad, torch.int32, (4, 4), "common int32 [M, M]")
    r.set(n_poses=4, min_size=2, cutoff_fcc=0.5)
    assert (r.q.n_poses, r.q.min_size, r.q.cutoff_fcc) == (4, 2, 0.5)
    with pytest.raises(AttributeError):                                # ctypes alone would take the misspelt name
        r.set(n_pose=4)
    assert r.stream() is None


def test_run_goes_through_the_api_method(api):
    from deeprank_gnn_amd import _lib
    from deeprank_gnn_amd._request import Request
    r = Request(_lib.PoseCommonRequest, "cpu")
    bits = torch.tensor([[3], [6], [0]], dtype=torch.int64)
    r.input("bits_a", bits)
    r.input("bits_b", bits)
    r.set(n_a=3, n_b=3, n_words=1)
    out = r.output("common", (3, 3), torch.int32)
    r.run(api, "pose_common")
    assert out.tolist() == [[2, 1, 0], [1, 2, 0], [0, 0, 0]]


# ---- the records ----------------------------------------------------------------------------------------------------
# host_<x> fields without a device copy <x> in the same record, and why there is none
HOST_ONLY = {("ScoreRequest", "host_zone_ptr"): "four offsets into zone_atom that only the host reads",
             ("EpochPlan", "host_node_ptr"): "the device copy is a member of the graph set `set` points to",
             ("EpochPlan", "host_edge_ptr"): "the device copy is a member of the graph set `set` points to",
             ("EpochPlan", "host_c1_ptr"): "the device copy is a member of the graph set `set` points to",
             ("StepHints", "host_node_ptr"): "hints on the host side of a launch: the device tables are launch arguments",
             ("StepHints", "host_edge_ptr"): "hints on the host side of a launch: the device tables are launch arguments",
             ("StepHints", "host_ids"): "hints on the host side of a launch: the device tables are launch arguments"}


def test_every_host_field_of_a_record_has_its_device_sibling():
    from deeprank_gnn_amd import _lib
    records = [c for c in vars(_lib).values() if isinstance(c, type) and issubclass(c, ctypes.Structure)]
    assert len(records) >= 25 and _lib.BsaRequest in records
    host_only = set()
    for c in records:
        names = [n for n, _ in c._fields_]
        for n in names:
            if n.startswith("host_") and n[len("host_"):] not in names:
                host_only.add((c.__name__, n))
    assert host_only == set(HOST_ONLY)
    assert {k for k in HOST_ONLY if k[0].endswith("Request")} == {("ScoreRequest", "host_zone_ptr")}


# ---- one place ------------------------------------------------------------------------------------------------------
# (file, object) whose host_* attributes are assigned outside the filler, and why that is no request record
ASSIGNED_ELSEWHERE = {("_lib.py", "h"): "step_hints: StepHints holds host tables only, pinned in its keep-alive tuple",
                      ("trainer.py", "plan"): "the epoch plan: host tables of the resident set and of its own ids, one owner",
                      ("topology.py", "self"): "numpy attributes of a Topology, not fields of a record",
                      ("topology.py", "topo"): "numpy attributes of a Topology, not fields of a record"}


def _host_assignments(text):
    """(object, line) of every assignment to an attribute whose name starts with host_, or names one through "host_" + ..."""
    found = []
    for line in text.split("\n"):
        code = line.split("#")[0]
        target = re.match(r"^((?:[^=!<>(]|\([^)]*\))*?)(?<![=!<>])=(?!=)", code)          # up to the first plain "="
        if target:
            found += [(obj, line) for obj in re.findall(r"(\w+)\.host_\w+", target.group(1))]
        if re.search(r"[\"']host_[\"']\s*\+|setattr\([^)]*host_", code):
            found.append(("<by name>", line))
    return found


def test_the_search_sees_the_ways_to_assign_a_host_field():
    seen = _host_assignments("q.host_a = 1\n    q.xyz, q.host_b, q.n = a, b, c\n(q.host_c,\n q.host_d) = x\n"
                             "piece = (plan.ids, plan.host_ids)\nif q.host_e == 3:\n    f(host_x=q.host_y)\n"
                             "setattr(q, 'host_' + k, v)\nself.set(**{\"host_\" + name: 1})\nq.a = q.host_z  # q.host_w = 1\n")
    assert [s[0] for s in seen] == ["q", "q", "q", "<by name>", "<by name>"]


def test_host_fields_are_assigned_in_the_filler_alone():
    files = sorted(glob.glob(os.path.join(PACKAGE, "*.py")))
    assert len(files) > 25
    where = set()
    for path in files:
        with open(path) as f:
            where |= {(os.path.basename(path), obj) for obj, _ in _host_assignments(f.read())}
    assert where == {("_request.py", "<by name>")} | set(ASSIGNED_ELSEWHERE)


# ---- the facade -----------------------------------------------------------------------------------------------------
# what deeprank_gnn_amd.interface defined before it was split: sorted(n for n in vars(interface) if not n.startswith("__")),
# modules left out
NAMES = ['AtomTable', 'BACKBONE', 'BSA', 'BSA_BACKBONE', 'BSA_FIRST_LETTER', 'BSA_SIDE_CHAIN', 'BSA_XYZ_BUDGET', 'ContactFrequency',
         'DEPTH', 'DEPTH_COMPONENTS', 'DEPTH_OTHER', 'DEPTH_UNITED', 'DEPTH_WORKSPACE_BUDGET', 'FCC_XYZ_BUDGET', 'FEATURES',
         'FEATURE_WIDTH', 'Feature', 'HSE', 'HSE_BACKBONE', 'HSE_CONNECT', 'HSE_DIRECTION', 'HSE_TILE', 'HSE_WORKGROUPS',
         'MCL_WORKSPACE_BUDGET', 'PACK_SOURCE', 'PoseClusters', 'PoseContacts', 'Poses', 'RESIDUE_CHARGE', 'RESIDUE_NAMES',
         'RESIDUE_POLARITY', 'RESIDUE_XYZ_BUDGET', 'RMSD_KINDS', 'RMSD_WORKSPACE_BUDGET', 'SCORE_KEYS', 'SCORE_XYZ_BUDGET',
         'ScoreReference', 'WORKSPACE_BUDGET', '_C', '_CR', '_CT', '_N', '_O1', '_O2', '_S', '_TYPE_OF', '_atom_list',
         '_blocked_pairs', '_bsa_graph_options', '_bsa_options', '_check_min_size', '_cluster_launch', '_common_device',
         '_complexes', '_contact_words', '_default_device', '_depth_graph_options', '_depth_options', '_depth_too_large',
         '_feature_chunk', '_group_rows', '_hse_graph_options', '_hse_node_data', '_hse_options', '_i32', '_mcl_groups',
         '_pack_columns', '_per_table', '_pose_batch', '_pose_clusters', '_ragged', '_residue_pairs', '_residue_tables',
         '_residue_values', '_targets', 'attach_residue_features', 'attach_scores', 'bsa_radii', 'bsa_raw', 'build_ragged',
         'build_ragged_device', 'cluster_poses', 'cluster_poses_rmsd', 'common_contacts', 'consensus_bits_raw',
         'consensus_contacts', 'consensus_numerators_raw', 'consensus_scores', 'contact_counts_raw', 'contact_frequency',
         'counted_atoms', 'default_chunk', 'depth_dots', 'depth_link', 'depth_radii', 'depth_raw', 'dock_scores_raw',
         'docking_scores', 'fcc_matrix', 'hse_raw', 'hse_table', 'hse_tile', 'iface_pack_raw', 'interface_graphs',
         'interface_resident_set', 'interface_residues', 'pack_request', 'pack_type_table', 'pose_cluster_dist_raw',
         'pose_cluster_raw', 'pose_common_raw', 'pose_contacts', 'pose_contacts_raw', 'pose_rmsd', 'pose_rmsd_raw',
         'read_pdb_atom_names', 'read_pdb_atoms', 'residue_bsa', 'residue_depth', 'residue_hse', 'rmsd_selection', 'select_atoms']
# the (host, device) pair helper of the consensus calls: the filler's ``table`` took its place, nothing stands in for it
REPLACED_BY_THE_FILLER = {"_i32"}
HOMES = ("atoms", "residue_features", "dock_scores", "iface_graphs", "poses")


def test_interface_still_exports_every_name_from_its_home_module():
    from deeprank_gnn_amd import interface
    assert len(NAMES) == 122 and NAMES == sorted(set(NAMES))
    defined = {}                                                       # name -> the modules whose source defines it
    for m in HOMES:
        with open(os.path.join(PACKAGE, m + ".py")) as f:
            for node in ast.parse(f.read()).body:
                targets = [node] if isinstance(node, (ast.FunctionDef, ast.ClassDef)) else getattr(node, "targets", [])
                for t in targets:
                    for leaf in ([t] if not isinstance(t, ast.Tuple) else t.elts):
                        defined.setdefault(getattr(leaf, "name", getattr(leaf, "id", None)), []).append(m)
    for name in NAMES:
        if name in REPLACED_BY_THE_FILLER:
            assert not hasattr(interface, name) and name not in defined
            continue
        assert len(defined.get(name, [])) == 1, (name, defined.get(name))
        home = importlib.import_module("deeprank_gnn_amd." + defined[name][0])
        assert getattr(interface, name) is getattr(home, name), name
    for cls in ("AtomTable", "Poses", "PoseContacts", "PoseClusters", "ContactFrequency", "ScoreReference"):
        assert getattr(interface, cls).__module__ in ["deeprank_gnn_amd." + m for m in HOMES]
    assert interface.__doc__.startswith("Interface graphs from atom coordinates")
    assert set(interface.PACK_SOURCE) == set(interface.FEATURE_WIDTH) == {"type", "polarity", "charge", "pos", "chain", "bsa", "hse",
                                                                          "depth"}


def test_the_modules_import_in_one_direction():
    allowed = {"atoms": set(), "_request": set(), "residue_features": {"atoms", "_request"}, "dock_scores": {"atoms", "_request"},
               "poses": {"atoms", "_request"}, "iface_graphs": {"atoms", "_request", "residue_features", "dock_scores"}}
    for module, may in allowed.items():
        with open(os.path.join(PACKAGE, module + ".py")) as f:
            text = f.read()
        at_top = set(re.findall(r"^from \.(\w+) import", text, re.M)) - {"_lib"}
        assert at_top <= may, (module, at_top)
        inside = set(re.findall(r"^\s+from \.(\w+) import", text, re.M))       # the lazy imports that were there before
        assert inside <= {"dataset", "clustering", "resident"}, (module, inside)


def test_the_package_imports_without_the_library_or_the_gpu():
    import deeprank_gnn_amd
    code = ("import torch, deeprank_gnn_amd\nfrom deeprank_gnn_amd import _lib, interface\n"
            "assert _lib._API is None and not torch.cuda.is_initialized()\n"
            "print(sorted(n for n in vars(deeprank_gnn_amd) if not n.startswith('_')))")
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    public = ["AtomTable", "ScoreReference", "attach_residue_features", "attach_scores", "bsa_radii", "cluster_poses",
              "cluster_poses_rmsd", "common_contacts", "consensus_contacts", "consensus_scores", "contact_frequency", "depth_radii",
              "docking_scores", "fcc_matrix", "hse_table", "interface_graphs", "interface_residues", "interface_resident_set",
              "pose_contacts", "pose_rmsd", "read_pdb_atom_names", "read_pdb_atoms", "residue_bsa", "residue_depth", "residue_hse",
              "select_atoms"]
    from deeprank_gnn_amd import interface
    for name in public:
        assert name in out.stdout and getattr(deeprank_gnn_amd, name) is getattr(interface, name), name


# ---- the table of entry points --------------------------------------------------------------------------------------
def test_every_registered_entry_point_is_a_method_of_api(api):
    from deeprank_gnn_amd import _lib
    assert len(_lib.REQUEST_CALLS) == 14 and len(_lib.CAPACITY_CALLS) == 7
    for name, symbol, record in _lib.REQUEST_CALLS:
        assert callable(vars(_lib.Api)[name]) and vars(_lib.Api)[name].__code__.co_varnames[:3] == ("self", "request", "stream")
        assert issubclass(record, ctypes.Structure)
        assert getattr(api.lib, symbol).argtypes == [ctypes.POINTER(record), ctypes.c_void_p]
    for name in _lib.CAPACITY_CALLS:
        assert callable(vars(_lib.Api)[name]) and isinstance(getattr(api, name)(0), int)
        assert getattr(api.lib, "drgnn_" + name).restype is ctypes.c_int32


def test_a_method_patched_on_the_class_is_what_the_interface_calls(api, monkeypatch):
    from deeprank_gnn_amd import interface
    t = interface.AtomTable(["A", "A", "B", "B"], [1, 2, 1, 2], ["ALA"] * 4, [[0, 0, 0], [30, 0, 0], [3, 0, 0], [60, 0, 0]])
    c = interface.pose_contacts(t, api=api, device="cpu")
    assert c.n_contacts.tolist() == [1]
    calls, real = [], type(api).pose_common
    monkeypatch.setattr(type(api), "pose_common", lambda self, q, stream: (calls.append((q.n_a, q.n_b)), real(self, q, stream))[1])
    assert interface.common_contacts(c).tolist() == [[1]] and calls == [(1, 1)]
    monkeypatch.setattr(type(api), "fcc_capacity", lambda self, what: 0)
    with pytest.raises(Exception, match="capacity"):
        interface.pose_contacts(t, api=api, device="cpu")
