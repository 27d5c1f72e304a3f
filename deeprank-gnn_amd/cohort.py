"""Training K members of one net (cross-validation folds, seeds, a learning-rate sweep) over ONE resident set.

The training counterpart of ``Ensemble``.  The reference's fold models are produced by K NeuralNet objects trained one after
the other, each reading the set again.  Here the set is uploaded once, its topology is cached once, and one optimisation step
of ALL K members is two launches: the fused cohort step (drgnn_cohort_train_step_cached: one workgroup per (member, graph),
the K members of a graph on the same XCD) and the cohort update (drgnn_cohort_update: the fixed-order slab sums and Adam,
once per member).  Each member has its own mini-batch (folds have different training sets: the sizes may differ, a member may
have none in a step and is then left alone), its own dropout stream, step index, learning rate and loss word.  Member m's
trajectory is that of a ``FusedTrainer`` of its own with the one-workgroup-per-graph layout, bit for bit.

The members are a members.MemberPack: nets and trainers on rows of packed ``[K, P]`` tensors (parameters, gradients, both
Adam moments); the member table (drgnn_cohort_member[K]) is written to the device when the buffers of a batch size are made.

``last_path`` / ``last_reason`` as ``Ensemble``: ``"fused"`` (every step in the cohort launches) or ``"separate"`` (the plan
answered NONE -- the host emulation, a graph beyond the fused kernels, no cached topology: each member runs its own step, one
after the other, with the same results).
"""
import ctypes

import numpy as np
import torch

from . import _lib
from .ensemble import Ensemble
from .functional import H2
from .launch import fused, head_desc, wrong_targets
from .members import MemberPack, checkpoint_state, device_table, fill_member, load_members

__all__ = ["Cohort", "kfold_indices"]


def kfold_indices(n, k, shuffle=True, seed=0):
    """k disjoint validation folds (int64 arrays) that cover ``range(n)``, sizes differing by at most one."""
    n, k = int(n), int(k)
    if k < 2 or k > n:
        raise ValueError("kfold_indices: need 2 <= k <= n (k = %d, n = %d)" % (k, n))
    idx = np.arange(n, dtype=np.int64)
    if shuffle:
        idx = np.random.RandomState(seed).permutation(n).astype(np.int64)
    return [np.sort(f) for f in np.array_split(idx, k)]


def _per_member(value, K, what, cast):
    if isinstance(value, (list, tuple, np.ndarray)):
        if len(value) != K:
            raise ValueError("Cohort: %s has %d entries for %d members" % (what, len(value), K))
        return [cast(v) for v in value]
    return [cast(value)] * K


def _per_member_tables(value, K):
    """``lr_schedule``: None, one table for all members, or K tables ([K, n]; an entry may be None)"""
    if value is None:
        return [None] * K
    if len(value) and isinstance(value[0], (list, tuple, np.ndarray, type(None))):
        if len(value) != K:
            raise ValueError("Cohort: lr_schedule has %d tables for %d members" % (len(value), K))
        return [None if t is None else [float(v) for v in t] for t in value]
    return [[float(v) for v in value]] * K


class Cohort(MemberPack):
    """K members of the net class ``Net``: ``members`` is K (fresh nets ``Net(n_feat, n_out, edge_dim)``) or a list of
    checkpoint paths / checkpoint dictionaries / state dicts to start from.  ``lr`` and ``seeds`` (dropout streams) are
    scalars or length-K lists; ``seeds=None`` gives every member a stream of its own.  ``weight_decay`` and
    ``max_grad_norm`` (None: off) likewise, ``lr_schedule`` one table or K of them; ``decoupled_weight_decay`` is the
    cohort's (FusedTrainer's options: they run inside the two cohort launches, a clipping member's Adam step in a third)."""

    def __init__(self, Net, members, n_feat=None, n_out=1, lr=0.01, task="reg", seeds=None, class_weights=None,
                 transform_sigmoid=False, device=None, api=None, edge_dim=1, betas=(0.9, 0.999), eps=1e-8,
                 weight_decay=0.0, decoupled_weight_decay=False, max_grad_norm=None, lr_schedule=None):
        if isinstance(members, (int, np.integer)):
            if members < 1 or n_feat is None:
                raise ValueError("Cohort: K >= 1 fresh members need n_feat")
            K, states = int(members), None
        else:
            states, sig = load_members(Net, members, "Cohort", {"task": task})
            K, n_feat, n_out = len(states), sig["F"], sig["O"]
        self.task, self.classes = task, None if task == "reg" else list(range(int(n_out)))
        self.transform_sigmoid = bool(transform_sigmoid) and task == "reg"
        self.lr = _per_member(lr, K, "lr", float)
        if seeds is None:
            seeds = [(torch.initial_seed() + m * 0x9E3779B1) & 0xFFFFFFFF for m in range(K)]
        self.seeds = _per_member(seeds, K, "seeds", lambda v: int(v) & 0xFFFFFFFF)
        self.weight_decay = _per_member(weight_decay, K, "weight_decay", float)
        self.max_grad_norm = _per_member(max_grad_norm, K, "max_grad_norm", lambda v: None if v is None else float(v))
        self.lr_schedule = _per_member_tables(lr_schedule, K)
        MemberPack.__init__(self, Net, K, n_feat, n_out, device, edge_dim, states=states, training=True,
                            per_member=[{"lr": self.lr[m], "seed": self.seeds[m], "weight_decay": self.weight_decay[m],
                                         "max_grad_norm": self.max_grad_norm[m], "lr_schedule": self.lr_schedule[m]}
                                        for m in range(K)], task=task,
                            class_weights=class_weights, betas=betas, eps=eps, api=api,
                            transform_sigmoid=self.transform_sigmoid, decoupled_weight_decay=decoupled_weight_decay)
        # [K] the members' gradient norms before clipping (each trainer's grad_norm word is its entry)
        self.grad_norm = torch.zeros(K, dtype=torch.float32, device=self.device)
        for m, tr in enumerate(self.trainers):
            tr._grad_norm = self.grad_norm[m:m + 1]
        self._optims, self._any_clip = None, False
        for tr in self.trainers:
            # the one-workgroup-per-graph layout, as the cohort launch: a member stepped on its own (the separate path)
            # gives the bits the cohort launch gives
            tr.plan_overrides = {"force_wgs": 1}
        self._g1, self._g2, self._desc0 = self.trainers[0]._descs(self.n_feat)
        self._cap, self._table, self._bufs = 0, None, None
        self.last_pred = [None] * K

    # -- members --------------------------------------------------------------------------------------------------------
    def state_dicts(self):
        return [{k: v.detach().cpu().clone() for k, v in tr.net.state_dict().items()} for tr in self.trainers]

    def save(self, paths, **settings):
        """K checkpoints in NeuralNet.save_model's dictionary layout (``settings``: its other entries -- node, edge, target,
        batch_size, ...): ``NeuralNet(db, Net, pretrained_model=paths)`` loads them as an ensemble."""
        paths = list(paths)
        if len(paths) != self.K:
            raise ValueError("Cohort.save: %d paths for %d members" % (len(paths), self.K))
        cw = self.trainers[0].class_w
        common = dict(node=None, edge=['dist'], target=None, task=self.task, classes=list(range(max(self.O, 2))),
                      class_weight=None if cw is None else cw.cpu().tolist(), batch_size=32, percent=[1.0, 0.0], index=None,
                      shuffle=True, threshold=0.3, cluster_nodes='mcl', transform_sigmoid=self.transform_sigmoid)
        for m, (path, sd) in enumerate(zip(paths, self.state_dicts())):
            torch.save(checkpoint_state(sd, self.trainers[m].optimizer_state_dict(),
                                        **{**common, 'lr': self.lr[m], **settings}), path)
        return paths

    def ensemble(self):
        """An ``Ensemble`` over the members' CURRENT parameters: it shares the cohort's parameter buffer (no copy), so it
        scores with whatever the cohort has trained so far."""
        return Ensemble.over(self)

    def faults(self):
        """the members' sticky fault words ([K] int32 view on the device)"""
        return self.step2[:, 2]

    def raise_on_faults(self):
        for m, bits in enumerate(self.faults().cpu().tolist()):
            if bits:
                try:
                    self.trainers[m].raise_on_faults(bits)
                except _lib.DrgnnError as exc:
                    raise _lib.DrgnnError("cohort member %d: %s" % (m, exc))

    # -- one step -------------------------------------------------------------------------------------------------------
    def plan(self, cache, ids, B):
        """drgnn_cohort_step_plan of a cohort launch of ``B`` graphs per member with the bounds of the graphs ``ids`` of
        ``cache``, and (bounds, flags, tiles) of that launch"""
        return self.member_plan(self.api.cohort_step_plan, cache, ids, B)

    def _ensure(self, B):
        """the members' outputs and slabs for mini-batches of up to ``B`` graphs, and the member table that names them
        (it caches each member's lr / betas / eps: changing a member's hyper-parameters after its first step is not supported)"""
        if B <= self._cap:
            return
        K, dev, api, nb = self.K, self.device, self.api, self.n_branch
        pred = torch.zeros((K, B, self.O), dtype=torch.float32, device=dev)
        readout = torch.empty((K, B, H2 * nb), dtype=torch.float32, device=dev)
        partials = torch.empty((K, B * nb, api.net_partial_elems(self.kind, self.n_feat)), dtype=torch.float32, device=dev)
        hp = torch.empty((K, B, api.head_compact_elems(self.R, self.H, self.O)), dtype=torch.float32, device=dev)
        table = (_lib.CohortMember * K)()
        for m, tr in enumerate(self.trainers):
            t = table[m]
            fill_member(t, tr, tr._descs(self.n_feat)[2])
            t.flat_param, t.flat_grad = tr.flat_p.data_ptr(), tr.flat_g.data_ptr()
            t.exp_avg, t.exp_avg_sq = tr.exp_avg.data_ptr(), tr.exp_avg_sq.data_ptr()
            t.step2, t.loss = tr.step2.data_ptr(), tr._loss_buf.data_ptr()
            t.pred, t.readout, t.head_partials, t.partials = pred[m].data_ptr(), readout[m].data_ptr(), hp[m].data_ptr(), partials[m].data_ptr()
            t.lr, t.beta1, t.beta2, t.eps, t.seed = tr.lr, tr.betas[0], tr.betas[1], tr.eps, tr.seed
        self._table = device_table(table, dev)
        self._bufs, self._cap = (pred, readout, partials, hp), B
        # the members' option records (drgnn_optim[K]) next to it, when any member has an option on
        self._optims = None
        if any(tr._optim() is not None for tr in self.trainers):
            records = (_lib.Optim * K)()
            for m, tr in enumerate(self.trainers):
                ctypes.memmove(ctypes.addressof(records[m]), ctypes.addressof(tr._optim(always=True)), ctypes.sizeof(_lib.Optim))
            self._optims = device_table(records, dev)
            self._any_clip = any(tr.max_grad_norm is not None for tr in self.trainers)

    def _tables(self, rs, batches):
        """``batches``: [steps][K] lists of graph numbers -> (ids [steps, K, B] int32, counts [steps, K] int32) on the
        device (one upload), B, and the host copies"""
        steps, K = len(batches), self.K
        B = max(1, max(len(b) for row in batches for b in row))
        ids = np.zeros((steps, K, B), dtype=np.int32)
        counts = np.zeros((steps, K), dtype=np.int32)
        for s, row in enumerate(batches):
            if len(row) != K:
                raise ValueError("Cohort: %d mini-batches for %d members" % (len(row), K))
            for m, b in enumerate(row):
                b = np.asarray(b, dtype=np.int64).reshape(-1)
                if b.size and (b.min() < 0 or b.max() >= len(rs)):
                    raise IndexError("graph number out of range [0, %d)" % len(rs))
                ids[s, m, :b.size] = b
                counts[s, m] = b.size
        both = torch.from_numpy(np.concatenate([ids.reshape(-1), counts.reshape(-1)]))
        if self.device.type == "cuda":
            both = both.pin_memory().to(self.device, non_blocking=True)
        return both[:ids.size].view(steps, K, B), both[ids.size:].view(steps, K), B, ids, counts

    def _launch(self, cache, memo, ids_ptr, counts_ptr, B, shared_ids=None, losses_ptr=None):
        """the two launches of one cohort step; ``memo``: what ``_prepare`` made for this run's launches"""
        p, bounds, flags, tiles, desc, head, (hints, _) = memo
        stream = _lib.current_stream(cache.set.x)      # (at launch time: a recorded hipGraph captures on a stream of its own)
        if shared_ids is not None:
            gset = cache.set
            hints, keep = _lib.step_hints(set_node_ptr=gset.node_ptr, set_edge_ptr=gset.edge_ptr, ids=shared_ids,
                                          topo_flags=flags, tiles=tiles, plan=p)
        api = self.api
        api.cohort_train_step_cached(self._desc0, head, self._table, self.K, desc, ids_ptr, counts_ptr, B, B,
                                     bounds[0], bounds[1], bounds[2], stream, hints)
        api.cohort_update(self._desc0, self._table, self.K, counts_ptr, self._g1, self._g2, self.R, self.H, self.O,
                          self.head_offset, self.n_param, stream, losses=losses_ptr, optims=self._optims,
                          any_clip=self._any_clip)

    def _prepare(self, cache, all_ids, B):
        """(plan, bounds, flags, tiles, cache descriptor, head descriptor, hints) of cohort launches of ``B`` graphs
        per member over graphs among ``all_ids``, or None when the plan answers NONE"""
        p, bounds, flags, tiles = self.plan(cache, all_ids, B)
        if not fused(p):
            return None
        self._ensure(B)
        tr0 = self.trainers[0]
        head = head_desc(tr0.net, tr0.task, True, getattr(tr0.net, "dropout", 0.0), tr0.seed, self.transform_sigmoid,
                         tr0.class_w)
        return (p, bounds, flags, tiles, cache.desc_for(self.kind == _lib.SGAT), head,
                _lib.step_hints(topo_flags=flags, tiles=tiles, plan=p))

    def _separate_step(self, rs, cache, row):
        """each member's own step on its mini-batch, one after the other (a member without one is left alone)"""
        from .topology import Topology
        for m, ids in enumerate(row):
            if len(ids) == 0:
                continue
            tr = self.trainers[m]
            ids = [int(i) for i in ids]
            try:
                if cache is None:
                    raise _lib.DrgnnError("no cached topology")
                tr.train_step_cached(cache, ids)
            except _lib.DrgnnError:
                batch = rs.batch(ids)
                tr.train_step(batch, topo=Topology.from_batch(batch, api=tr.api, need_weights=self.kind == _lib.SGAT))
            self.last_pred[m] = tr.last_pred

    def _run(self, rs, batches, cached=None):
        """``batches``: [steps][K] lists of graph numbers.  Returns the losses [steps, K] (NaN where a member had no
        mini-batch), on the device, without synchronising."""
        wrong = wrong_targets(self.task == "reg", rs.y)
        if wrong:
            raise ValueError(wrong)
        steps, K = len(batches), self.K
        out = torch.full((steps, K), float("nan"), dtype=torch.float32, device=self.device)
        if steps == 0:
            return out
        step, reason, cache = self.stage(rs, batches, cached)
        if step is None:
            for s, row in enumerate(batches):
                self._separate_step(rs, cache, row)
                stepped = [m for m in range(K) if len(row[m])]
                if stepped:
                    out[s, stepped] = self.losses[stepped]
            self.last_path = "separate"
            self.last_reason = reason + ": each member's own launches, one after the other"
            return out
        lp = out.data_ptr()
        for s in range(steps):
            step(s, lp + 4 * s * K)
        self.last_pred = [self._bufs[0][m, :int(step.counts[steps - 1, m])] for m in range(K)]
        self.last_path, self.last_reason = "fused", reason
        return out

    def stage(self, rs, batches, cached=None):
        """Upload the mini-batches ``batches`` ([steps][K] lists of graph numbers) once and plan their launches.  Returns
        (step, reason, cache): ``step(s, losses_ptr=None)`` enqueues the two launches of step ``s`` on the current stream
        (no allocation, no synchronisation: capturable in a hipGraph), or None when the cohort launches do not take these
        mini-batches (``reason`` says why; ``_run`` then steps the members one by one)."""
        K = self.K
        if cached is None:
            cached = self._cached_ok(rs)
        if not cached:
            return None, "no cached topology", None
        if any(tr._coupled() for tr in self.trainers):
            return None, "coupled L2 weight decay (the flat Adam launch alone knows it)", rs.topology_cache(need_weights=self.kind == _lib.SGAT)
        cache = rs.topology_cache(need_weights=self.kind == _lib.SGAT)
        dev_ids, dev_counts, B, ids, counts = self._tables(rs, batches)
        used = np.unique(ids[np.arange(B)[None, None, :] < counts[:, :, None]])
        memo = self._prepare(cache, used, B) if used.size else None
        if memo is None:
            return None, "the plan of the cohort launch answered NONE for these graphs", cache
        # host-known sizes travel in the launch arguments only when ALL members step the same graphs (seeds, sweeps)
        same = B <= 64 and bool((counts == counts[:, :1]).all()) and bool((ids == ids[:, :1, :]).all())
        ip, cp = dev_ids.data_ptr(), dev_counts.data_ptr()

        def step(s, losses_ptr=None):
            shared = ids[s, 0, :B] if (same and counts[s, 0] == B) else None
            self._launch(cache, memo, ip + 4 * s * K * B, cp + 4 * s * K, B, shared, losses_ptr)
        step.counts, step.keep, step.plan = counts, (dev_ids, dev_counts), memo[0]
        return step, "two launches per step of all members (drgnn_cohort_train_step_cached + drgnn_cohort_update)", cache

    def train_step(self, cache_or_set, ids_per_member, cached=None):
        """One optimisation step of every member on its own mini-batch ``ids_per_member[m]`` (graph numbers of the resident
        set; an empty list leaves that member alone).  Returns ``losses`` ([K] on the device)."""
        rs = getattr(cache_or_set, "set", cache_or_set)
        self._run(rs, [[list(b) for b in ids_per_member]], cached)
        return self.losses

    def train_epoch(self, rs, orders, batch_size, cached=None):
        """One epoch of every member: ``orders[m]`` is member m's visiting order (graph numbers of ``rs``).  The ids are
        uploaded once, the steps are issued from here without synchronising.  Returns the losses of every step,
        [steps, K] on the device (NaN where a member had run out of mini-batches)."""
        if len(orders) != self.K:
            raise ValueError("Cohort.train_epoch: %d orders for %d members" % (len(orders), self.K))
        orders = [[int(i) for i in o] for o in orders]
        steps = max((len(o) + batch_size - 1) // batch_size for o in orders) if orders else 0
        batches = [[o[s * batch_size:(s + 1) * batch_size] for o in orders] for s in range(steps)]
        return self._run(rs, batches, cached)
