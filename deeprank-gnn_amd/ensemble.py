"""Inference with K checkpoints of one net (cross-validation folds, seeds) over ONE resident set.

The reference scores a docking set with its ten fold models by building ten NeuralNet objects and running ten test passes,
each of which reads and collates the set again.  Here the set is uploaded once (resident.ResidentGraphSet), its topology is
cached once, and per mini-batch ONE launch runs all K members (drgnn_ens_predict_cached: one workgroup per (model, graph),
the K models of a graph on the same XCD, so the graph's topology, tiles and node rows are read once into that L2).  The
members are a members.MemberPack: nets and inference-only trainers on the rows of one packed [K, P] parameter buffer; the
member table that names them is written to the device once, when the ensemble is built.  Each member's outputs are those
of the same model alone, bit for bit, with the one-workgroup-per-graph layout (the plan's force_wgs = 1).

``last_path`` / ``last_reason`` tell which path the last ``predict`` took, as StepEngine does: ``"fused"`` (every mini-batch
in one ensemble launch), ``"separate"`` (the members' own launches, one after the other: the plan answers NONE -- the host
emulation, a graph beyond the fused kernels, no cached topology) or ``"mixed"``.
"""
import numpy as np
import torch

from . import _lib
from .launch import fused, head_desc, set_hints
from .members import MemberPack, device_table, fill_member, load_members


class Ensemble(MemberPack):
    """K members of the net class ``Net`` (checkpoint paths, checkpoint dictionaries or state dicts), inference only.

    ``predict`` returns ``[K, n, O]`` on the device: the members' outputs as each alone would give them (after the sigmoid
    when the checkpoints set ``transform_sigmoid``; logits for classification)."""

    def __init__(self, Net, checkpoints_or_state_dicts, device=None, api=None, edge_dim=1):
        states, sig = load_members(Net, list(checkpoints_or_state_dicts), "Ensemble")
        self._build(Net, len(states), sig["F"], sig["O"], sig["task"], sig["classes"], sig["transform_sigmoid"], device, api,
                    edge_dim, states=states)

    @classmethod
    def over(cls, pack):
        """An ensemble over the CURRENT parameters of ``pack`` (a Cohort, another Ensemble): nets and trainers of its own
        (their default launch plans, their own step words) on the rows of ``pack.params``, no copy."""
        ens = cls.__new__(cls)
        ens._build(pack.Net, pack.K, pack.n_feat, pack.O, pack.task, pack.classes, pack.transform_sigmoid, pack.device,
                   pack.api, pack.edge_dim, params=pack.params)
        return ens

    def _build(self, Net, K, n_feat, n_out, task, classes, transform_sigmoid, device, api, edge_dim, **storage):
        self.task, self.classes, self.transform_sigmoid = task, classes, transform_sigmoid
        MemberPack.__init__(self, Net, K, n_feat, n_out, device, edge_dim, task=task, api=api,
                            transform_sigmoid=transform_sigmoid, **storage)
        tr0 = self.trainers[0]
        self._desc0 = tr0._descs(self.n_feat)[2]       # (the launch checks the members' layout against member 0's)
        self._head = head_desc(tr0.net, tr0.task, False, 0.0, tr0.seed, transform_sigmoid)
        # the member table (drgnn_ens_member[K]) in device memory, written once
        table = (_lib.EnsMember * self.K)()
        for m, tr in enumerate(self.trainers):
            fill_member(table[m], tr, tr._descs(self.n_feat)[2])
        self.table = device_table(table, self.device)

    def _resident(self, dataset):
        from .resident import ResidentGraphSet
        return dataset if isinstance(dataset, ResidentGraphSet) else ResidentGraphSet(dataset, self.device, api=self.api)

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
        return self.member_plan(self.api.ens_step_plan, cache, ids, len(ids))

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
        self.api.ens_predict_cached(self._desc0, self._head, self.table, self.K, cache.desc_for(self.kind == _lib.SGAT),
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
