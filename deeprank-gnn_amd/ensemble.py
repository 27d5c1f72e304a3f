"""Inference with K checkpoints of one net (cross-validation folds, seeds) over ONE resident set.

The reference scores a docking set with its ten fold models by building ten NeuralNet objects and running ten test passes,
each of which reads and collates the set again.  Here the set is uploaded once (resident.ResidentGraphSet), its topology is
cached once, and per mini-batch ONE launch runs all K members (drgnn_ens_predict_cached: one workgroup per (model, graph),
the K models of a graph on the same XCD, so the graph's topology, tiles and node rows are read once into that L2).  The
member table -- member m's conv parameters and head, rows of one packed [K, P] parameter buffer -- is written to the device
once, when the ensemble is built.  Each member's outputs are those of the same model alone, bit for bit, with the
one-workgroup-per-graph layout (the plan's force_wgs = 1).

``last_path`` / ``last_reason`` tell which path the last ``predict`` took, as StepEngine does: ``"fused"`` (every mini-batch
in one ensemble launch), ``"separate"`` (the members' own launches, one after the other: the plan answers NONE -- the host
emulation, a graph beyond the fused kernels, no cached topology) or ``"mixed"``.
"""
import numpy as np
import torch

from . import _lib
from .functional import _describe
from .launch import NetLayout, cached_flags, fused, head_desc, set_hints
from .trainer import FusedTrainer

# the properties the members of an ensemble must share (the ValueError names the first that differs)
KEYS = ("net", "F", "task", "O", "classes", "transform_sigmoid", "head")


def _load(member):
    """(model state dict, checkpoint settings) of a checkpoint path, a checkpoint dictionary (NeuralNet.save_model's) or a
    bare state dict."""
    if isinstance(member, (str, bytes)) or hasattr(member, "__fspath__"):
        member = torch.load(member, map_location="cpu", weights_only=False)
    if not isinstance(member, dict):
        raise TypeError("an ensemble member is a checkpoint path, a checkpoint dictionary or a state dict, not %r"
                        % type(member).__name__)
    if "model" in member and isinstance(member["model"], dict):
        return member["model"], member
    return member, {}


def _n_feat(Net, sd):
    """F of a state dict of one of the three nets (the in-features of its first layer)."""
    name = Net.__name__
    if name == "GINet":
        return int(sd["conv1.fc.weight"].shape[1])
    if name == "sGAT":
        return int(sd["conv1.weight"].shape[0]) // 2
    if name == "FoutNet":
        return int(sd["conv1.Wc"].shape[0])
    raise ValueError("Ensemble: unknown net class %s" % name)


def _signature(Net, sd, ck):
    O = int(sd["fc2.weight"].shape[0])
    task = ck.get("task") or ("reg" if O == 1 else "class")
    return {"net": Net.__name__, "F": _n_feat(Net, sd), "task": task, "O": O,
            "classes": None if task == "reg" else list(ck.get("classes", range(O))),
            "transform_sigmoid": bool(ck.get("transform_sigmoid", False)) and task == "reg",
            "head": (tuple(sd["fc1.weight"].shape), tuple(sd["fc2.weight"].shape)),
            "params": {k: tuple(v.shape) for k, v in sd.items()}}


def _first_difference(a, b):
    """the first key of the signatures a, b that differs (a parameter's name for the parameter shapes)"""
    for key in KEYS:
        if a[key] != b[key]:
            return key, a[key], b[key]
    for name in sorted(set(a["params"]) | set(b["params"])):
        if a["params"].get(name) != b["params"].get(name):
            return name, a["params"].get(name), b["params"].get(name)
    return None


class Ensemble(object):
    """K members of the net class ``Net`` (checkpoint paths, checkpoint dictionaries or state dicts), inference only.

    ``predict`` returns ``[K, n, O]`` on the device: the members' outputs as each alone would give them (after the sigmoid
    when the checkpoints set ``transform_sigmoid``; logits for classification)."""

    def __init__(self, Net, checkpoints_or_state_dicts, device=None, api=None, edge_dim=1):
        members = list(checkpoints_or_state_dicts)
        if not members:
            raise ValueError("Ensemble: no members")
        self.device = torch.device(device if device is not None else ("cuda" if torch.cuda.is_available() else "cpu"))
        loaded = [_load(m) for m in members]
        sigs = [_signature(Net, sd, ck) for sd, ck in loaded]
        for k, s in enumerate(sigs[1:], start=1):
            diff = _first_difference(s, sigs[0])
            if diff is not None:
                raise ValueError("Ensemble: member %d differs from member 0 in %r (%r against %r)" % ((k,) + diff))
        sig = sigs[0]
        self.Net, self.K, self.n_feat, self.O = Net, len(members), sig["F"], sig["O"]
        self.task, self.classes, self.transform_sigmoid = sig["task"], sig["classes"], sig["transform_sigmoid"]
        self.trainers = []
        for sd, _ in loaded:
            net = Net(self.n_feat, self.O, edge_dim)
            net.load_state_dict(sd, strict=True)
            tr = FusedTrainer(net.to(self.device), task=self.task, api=api, transform_sigmoid=self.transform_sigmoid)
            tr.exp_avg = tr.exp_avg_sq = None          # inference only: no optimiser state
            self.trainers.append(tr)
        tr0 = self.trainers[0]
        lay = NetLayout(tr0.net)
        # the K parameter sets packed in ONE device buffer [K, P] (the members' parameters are views of their rows)
        self.params = torch.stack([tr.flat_p for tr in self.trainers])
        for m, tr in enumerate(self.trainers):
            tr.flat_p = self.params[m]
            with torch.no_grad():
                lay.bind(tr.net, self.params[m])
        self.kind, self.api, self.n_branch = lay.kind, tr0.api, lay.n_branch
        self.R, self.H = lay.R, lay.H
        self._head = head_desc(tr0.net, _lib.TASK_REG if self.task == "reg" else _lib.TASK_CLASS, False, 0.0, tr0.seed,
                               self.transform_sigmoid)
        # the member table (drgnn_ens_member[K]) in device memory, written once; the host descriptors it was made from keep
        # the layout the launch checks against (member 0's)
        table = (_lib.EnsMember * self.K)()
        self._descs = []
        for m, tr in enumerate(self.trainers):
            d = _describe(self.kind, self.n_feat, tr.live, self.n_branch)
            self._descs.append(d)
            n = tr.net
            table[m].net = d
            table[m].w1, table[m].b1 = n.fc1.weight.data_ptr(), n.fc1.bias.data_ptr()
            table[m].w2, table[m].b2 = n.fc2.weight.data_ptr(), n.fc2.bias.data_ptr()
        self.table = torch.frombuffer(bytearray(bytes(table)), dtype=torch.uint8).to(self.device)
        self.last_path, self.last_reason = None, None

    @property
    def nets(self):
        return [tr.net for tr in self.trainers]

    def _resident(self, dataset):
        from .resident import ResidentGraphSet
        return dataset if isinstance(dataset, ResidentGraphSet) else ResidentGraphSet(dataset, self.device, api=self.api)

    def _cached_ok(self, rs):
        need_w = self.kind == _lib.SGAT
        return bool(rs.has_c0 and rs.has_c1) and not (need_w and rs.edge_attr is None)

    @torch.no_grad()
    def predict(self, dataset, indices=None, batch_size=64, cached=None):
        """``[K, n, O]`` predictions of the members on the graphs ``indices`` (default: all) of ``dataset`` (a
        ResidentGraphSet, or a graph dataset that is uploaded once for all members), mini-batches of ``batch_size``.
        ``cached``: read the set's cached topology (default: whenever the set carries both cluster levels); the fused
        ensemble launch reads it, without it the members are run one by one."""
        rs = self._resident(dataset)
        order = list(range(len(rs))) if indices is None else [int(i) for i in indices]
        n = len(order)
        out = torch.empty((self.K, n, self.O), dtype=torch.float32, device=self.device)
        if not order:
            return out
        if cached is None:
            cached = self._cached_ok(rs)
        if not cached:
            for m, tr in enumerate(self.trainers):
                pred = tr.predict_epoch(rs, order, batch_size, cached=False)
                if pred is None:
                    pred = self._predict_batches(tr, rs, order, batch_size)
                out[m].copy_(pred.reshape(n, self.O))
            self.last_path = "separate"
            self.last_reason = "no cached topology: the members' own launches, one after the other"
            return out
        cache = rs.topology_cache(need_weights=self.kind == _lib.SGAT)
        ids_dev = rs.upload_ids(order)
        fused = 0
        for lo in range(0, n, batch_size):
            ids = order[lo:lo + batch_size]
            dev_ids = ids_dev[lo:lo + batch_size]
            got = self._launch(cache, ids, dev_ids)
            if got is not None:
                fused += 1
                out[:, lo:lo + len(ids)].copy_(got)
            else:
                for m, tr in enumerate(self.trainers):
                    out[m, lo:lo + len(ids)].copy_(tr.predict_cached(cache, ids, dev_ids))
        n_batches = (n + batch_size - 1) // batch_size
        if fused == n_batches:
            self.last_path, self.last_reason = "fused", "one ensemble launch per mini-batch (drgnn_ens_predict_cached)"
        else:
            self.last_path = "separate" if fused == 0 else "mixed"
            self.last_reason = ("%d of %d mini-batches in the ensemble launch; the plan answered NONE for the others "
                                "(their members were launched one by one)" % (fused, n_batches))
        return out

    def plan(self, cache, ids):
        """drgnn_ens_step_plan of the ensemble launch over the graphs ``ids`` of ``cache`` (with the topology flags and tiles
        that launch reads), and those (flags, tiles)"""
        max_nodes, max_edges, max_c0 = cache.bounds(ids)
        flags, tiles = cached_flags(self.kind, cache)
        p = self.api.ens_step_plan(self.K, self.kind, self.n_feat, max_nodes, max_edges, max_c0, self.R, self.H, self.O,
                                   len(ids), flags)
        return p, (max_nodes, max_edges, max_c0), flags, tiles

    def _launch(self, cache, ids, ids_dev):
        """[K, B, O] of ONE ensemble launch over the graphs ``ids``, or None when its plan is NONE"""
        ids = np.asarray(ids, dtype=np.int64).reshape(-1)
        p, (mn, me, mc), flags, tiles = self.plan(cache, ids)
        if not fused(p):
            return None
        B, gset = int(ids.size), cache.set
        pred = torch.empty((self.K, B, self.O), dtype=torch.float32, device=self.device)
        readout = torch.empty((self.K, B, self.R), dtype=torch.float32, device=self.device)
        hints = set_hints(gset, ids, flags, tiles, p)
        self.api.ens_predict_cached(self._descs[0], self._head, self.table, self.K, cache.desc_for(self.kind == _lib.SGAT),
                                    ids_dev, B, mn, me, mc, self.trainers[0].step2, pred, readout, _lib.current_stream(gset.x),
                                    hints[0])
        return pred

    def _predict_batches(self, tr, rs, order, batch_size):
        """per-mini-batch path of one member (graphs the native loop does not take), as NeuralNet.eval runs it"""
        from .topology import Topology
        need_w = self.kind == _lib.SGAT
        ids_dev = rs.upload_ids(order)
        preds = []
        for lo in range(0, len(order), batch_size):
            batch = rs.batch(order[lo:lo + batch_size], ids_dev[lo:lo + batch_size])
            topo = Topology.from_batch(batch, api=tr.api, need_weights=need_w)
            preds.append(tr.predict(batch, topo=topo).clone())
        return torch.cat(preds)

    def combine(self, preds):
        """(mean, per-member outputs) of ``[K, n, O]`` predictions: for regression the mean of the members' outputs
        and ``[n, K]``; for classification the mean of their softmax probabilities ``[n, O]`` and ``[n, K, O]``."""
        if self.task == "class":
            prob = torch.softmax(preds, dim=2)
            return prob.mean(dim=0), prob.permute(1, 0, 2).contiguous()
        per = preds.reshape(self.K, -1).t().contiguous()
        return per.mean(dim=1), per

    def faults(self):
        return [tr.step2[2:3] for tr in self.trainers]

    def raise_on_faults(self):
        for tr in self.trainers:
            tr.check_faults()
