"""K members of one net (cross-validation folds, seeds, a sweep) over packed storage: what ``Ensemble`` (inference) and
``Cohort`` (training) are both built on.

A member is a checkpoint path, a checkpoint dictionary (``checkpoint_state``) or a bare state dict; ``load_members`` reads K of
them and checks that they are one net.  ``MemberPack`` makes the K nets and their FusedTrainers and puts every trainer on its
row of packed ``[K, P]`` tensors through ``FusedTrainer.adopt_storage``.  A member table is K C structs in device memory that
name those rows: ``fill_member`` writes the fields the two table types share, ``device_table`` uploads them.
"""
import torch

from . import _lib
from .launch import cached_flags
from .trainer import FusedTrainer

# the properties the members must share (the ValueError names the first that differs)
KEYS = ("net", "F", "task", "O", "classes", "transform_sigmoid", "head")
# a checkpoint's entries besides 'model' and 'optimizer' (NeuralNet reads every one of them back)
SETTINGS = ("node", "edge", "target", "task", "classes", "class_weight", "batch_size", "percent", "lr", "index", "shuffle",
            "threshold", "cluster_nodes", "transform_sigmoid", "weight_decay", "decoupled_weight_decay", "max_grad_norm",
            "lr_schedule")


def checkpoint_state(model_sd, optimizer_sd, **settings):
    """The checkpoint dictionary of NeuralNet.save_model (the reference's, NeuralNet.py:776); ``settings``: SETTINGS."""
    return dict({"model": model_sd, "optimizer": optimizer_sd}, **settings)


def _load(member):
    """(model state dict, checkpoint settings) of a checkpoint path, a checkpoint dictionary (NeuralNet.save_model's) or a
    bare state dict."""
    if isinstance(member, (str, bytes)) or hasattr(member, "__fspath__"):
        member = torch.load(member, map_location="cpu", weights_only=False)
    if not isinstance(member, dict):
        raise TypeError("a member is a checkpoint path, a checkpoint dictionary or a state dict, not %r"
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
    raise ValueError("unknown net class %s" % name)


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


def load_members(Net, members, owner, settings=None):
    """(state dicts, member 0's signature) of the ``members`` of ``owner`` ("Ensemble" / "Cohort": the prefix of its
    errors), which must agree in KEYS and in every parameter's shape.  ``settings``: read the task, classes and sigmoid
    from this dictionary instead of each member's checkpoint."""
    loaded = [_load(m) for m in members]
    if not loaded:
        raise ValueError("%s: no members" % owner)
    sigs = [_signature(Net, sd, ck if settings is None else settings) for sd, ck in loaded]
    for k, s in enumerate(sigs[1:], start=1):
        diff = _first_difference(s, sigs[0])
        if diff is not None:
            raise ValueError("%s: member %d differs from member 0 in %r (%r against %r)" % ((owner, k) + diff))
    return [sd for sd, _ in loaded], sigs[0]


def fill_member(entry, trainer, desc):
    """the fields an ensemble's and a cohort's table entry share: the net descriptor ``desc`` and the head's parameters"""
    n = trainer.net
    entry.net = desc
    entry.w1, entry.b1 = n.fc1.weight.data_ptr(), n.fc1.bias.data_ptr()
    entry.w2, entry.b2 = n.fc2.weight.data_ptr(), n.fc2.bias.data_ptr()


def device_table(array, device):
    """the ctypes array ``array`` of member structs as bytes in device memory"""
    return torch.frombuffer(bytearray(bytes(array)), dtype=torch.uint8).to(device)


class MemberPack(object):
    """K nets ``Net(n_feat, n_out, edge_dim)`` (``states[m]``: member m's state dict; None: fresh nets) on ``device`` and
    a FusedTrainer each (``trainer_kw``: its arguments; ``per_member[m]``: member m's own on top), every trainer on row m of
    the packed tensors.

    ``params``: an existing ``[K, P]`` parameter tensor to put the members on (nothing is copied: the nets take whatever it
    holds); None: it is made by stacking the members' parameters.  ``training``: also ``grads``,
    ``exp_avg``, ``exp_avg_sq`` ([K, P]), ``step2`` ([K, 4]) and ``losses`` ([K]), zero; without it the trainers are
    inference only and keep step words of their own."""

    def __init__(self, Net, K, n_feat, n_out, device, edge_dim=1, states=None, params=None, training=False,
                 per_member=None, **trainer_kw):
        self.device = torch.device(device if device is not None else ("cuda" if torch.cuda.is_available() else "cpu"))
        self.Net, self.K, self.n_feat, self.O, self.edge_dim = Net, int(K), int(n_feat), int(n_out), edge_dim
        self.trainers = []
        for m in range(self.K):
            net = Net(self.n_feat, self.O, edge_dim)
            if states is not None:
                net.load_state_dict(states[m], strict=True)
            self.trainers.append(FusedTrainer(net.to(self.device), **dict(trainer_kw, **(per_member[m] if per_member else {}))))
        tr0 = self.trainers[0]
        lay = tr0.layout
        self.kind, self.api, self.n_branch, self.R, self.H = lay.kind, tr0.api, lay.n_branch, lay.R, lay.H
        self.head_offset, self.n_param = lay.head_offset, lay.total
        self.params = torch.stack([tr.flat_p for tr in self.trainers]) if params is None else params
        self.grads = self.exp_avg = self.exp_avg_sq = self.step2 = self.losses = None
        if training:
            self.grads, self.exp_avg, self.exp_avg_sq = (torch.zeros_like(self.params) for _ in range(3))
            self.step2 = torch.zeros((self.K, 4), dtype=torch.int32, device=self.device)
            self.losses = torch.zeros(self.K, dtype=torch.float32, device=self.device)
        for m, tr in enumerate(self.trainers):
            tr.adopt_storage(self.params[m], *((self.grads[m], self.exp_avg[m], self.exp_avg_sq[m], self.step2[m],
                                                self.losses[m:m + 1]) if training else ()))
        self.last_path, self.last_reason = None, None

    @property
    def nets(self):
        return [tr.net for tr in self.trainers]

    def _cached_ok(self, rs):
        """whether the members' launches can read the cached topology of the resident set ``rs``"""
        return bool(rs.has_c0 and rs.has_c1) and not (self.kind == _lib.SGAT and rs.edge_attr is None)

    def member_plan(self, api_fn, cache, ids, n_graphs):
        """(plan, bounds, flags, tiles) of a K-member launch of ``n_graphs`` graphs per member with the bounds of the graphs
        ``ids`` of ``cache``; ``api_fn``: the library's plan query of that launch"""
        bounds = cache.bounds(ids)
        flags, tiles = cached_flags(self.kind, cache)
        p = api_fn(self.K, self.kind, self.n_feat, bounds[0], bounds[1], bounds[2], self.R, self.H, self.O, n_graphs, flags)
        return p, bounds, flags, tiles
