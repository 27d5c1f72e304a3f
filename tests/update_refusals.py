"""What the update entry points refuse, and with which code (include/drgnn.h: drgnn_train_update, drgnn_step_update, their
``_opt`` twins, drgnn_cohort_update[_opt], drgnn_step_gradients, drgnn_net_reduce_grads).

Every case starts from ONE valid call of its entry point -- the smallest net descriptor the library accepts (GINet, one
branch, one feature) with two graphs, host buffers of the right sizes -- and alters exactly one argument or record member.
The refusals return before any device call, so they run on the product library without a GPU as well as on the emulation
build; the valid calls themselves run on the emulation build only (they show that a refusal comes from the altered member).
The codes are the ones recorded on the tree before the update launches got their call record.  Calls with two faults at
once are not pinned: the order of the checks is free.
"""
import ctypes
import re

import numpy as np

from deeprank_gnn_amd._lib import CohortMember, ConvGrads, NetDesc, Optim

E_ARG, E_CAPACITY, E_WIDTH = -1, -2, -3
H1, H2, MAX_OUT, ZERO_RANGES = 16, 32, 16, 8          # DRGNN_H1, DRGNN_H2, DRGNN_MAX_OUT, DRGNN_ZERO_RANGES
F, R, H, O, B, K = 1, H2, 1, 1, 2, 2
N_PARTIAL = 2 * F * H1 + H1 + 2 * H1 * H2 + H2          # net_partial_floats
HEAD_GRAD = H * R + H + O * H + O                       # the head's gradient block: dW1, db1, dW2, db2
HEAD_OFFSET = F * H1 + H1 * H2                          # flat layout: conv1.w_nbr, conv2.w_nbr, the head
N_PARAM = HEAD_OFFSET + HEAD_GRAD

_UPDATE_TAIL = "R H O head_offset flat_param flat_grad exp_avg exp_avg_sq n_param step loss"
_SOURCES = "net conv_partials n_graphs g_conv1 g_conv2 head_partials"
SIGS = {name: sig.split() for name, sig in {
    "train_update": _SOURCES + " head_slabs " + _UPDATE_TAIL + " lr beta1 beta2 eps apply_adam stream",
    "step_update": _SOURCES + " readout " + _UPDATE_TAIL + " lr beta1 beta2 eps apply_adam slabs_per_graph stream",
    "train_update_opt": _SOURCES + " head_slabs " + _UPDATE_TAIL + " optim apply_adam stream",
    "step_update_opt": _SOURCES + " readout " + _UPDATE_TAIL + " optim apply_adam slabs_per_graph stream",
    "cohort_update": "net members K counts g_conv1 g_conv2 R H O head_offset n_param losses apply_adam stream",
    "cohort_update_opt": "net members optims K counts g_conv1 g_conv2 R H O head_offset n_param losses apply_adam any_clip stream",
    "step_gradients": _SOURCES + " readout R H O head_grad graph_weight zero_ptr zero_len n_zero step slabs_per_graph stream",
    "net_reduce_grads": "net conv_partials n_nodes n_graphs g_conv1 g_conv2 grad_x stream",
}.items()}


def _addr(a):
    return a.ctypes.data


class World(object):
    """the operands of one valid call of every entry point (kept alive for the call)"""

    def __init__(self):
        f32 = lambda n: np.zeros(n, np.float32)                       # noqa: E731
        self.w1, self.w2 = f32(F * H1), f32(H1 * H2)
        self.flat_param, self.flat_grad, self.exp_avg, self.exp_avg_sq = (f32(N_PARAM) for _ in range(4))
        self.conv_partials = f32(2 * B * N_PARTIAL)                   # (room for the split layout's two slabs per graph)
        self.head_partials = f32(B * (HEAD_GRAD + 2))                 # (legacy slabs; the compact ones are smaller)
        self.readout, self.graph_weight = f32(B * R), f32(B)
        self.step, self.loss, self.losses = np.zeros(4, np.int32), f32(1), f32(K)
        self.head_grad, self.cleared = f32(HEAD_GRAD), f32(4)
        self.norm_words = np.zeros(64, np.float64)
        self.counts = np.full(K, B, np.int32)
        self.net = NetDesc()
        self.net.kind, self.net.n_branch, self.net.n_feat = 0, 1, F
        self.net.conv1[0].w_nbr, self.net.conv1[0].nbr_sk, self.net.conv1[0].nbr_sh = _addr(self.w1), H1, 1
        self.net.conv2[0].w_nbr, self.net.conv2[0].nbr_sk, self.net.conv2[0].nbr_sh = _addr(self.w2), H2, 1
        self.g1, self.g2 = (ConvGrads * 2)(), (ConvGrads * 2)()
        self.g1[0].w_nbr, self.g2[0].w_nbr = _addr(self.flat_grad), _addr(self.flat_grad) + 4 * F * H1
        self.optim = Optim()
        self.optim.lr, self.optim.beta1, self.optim.beta2, self.optim.eps = 1e-3, 0.9, 0.999, 1e-8
        self.optim.max_grad_norm, self.optim.norm_words, self.optim.norm_cap = 1.0, _addr(self.norm_words), 64
        self.optim.n_dead = 1                                         # (one empty dead range: its members are then checked)
        self.members, self.optims = (CohortMember * K)(), (Optim * K)()
        self.zero_ptr = (ctypes.c_void_p * ZERO_RANGES)(_addr(self.cleared))
        self.zero_len = (ctypes.c_int64 * ZERO_RANGES)(4)

    def values(self):
        v = {k: _addr(getattr(self, k)) for k in ("conv_partials", "head_partials", "readout", "flat_param", "flat_grad", "exp_avg",
                                                  "exp_avg_sq", "step", "loss", "losses", "counts", "head_grad", "graph_weight")}
        v.update(net=ctypes.byref(self.net), g_conv1=self.g1, g_conv2=self.g2, optim=ctypes.byref(self.optim),
                 members=ctypes.addressof(self.members), optims=ctypes.addressof(self.optims), K=K,
                 zero_ptr=self.zero_ptr, zero_len=self.zero_len, n_zero=1,
                 n_graphs=B, n_nodes=0, grad_x=None, head_slabs=1, R=R, H=H, O=O, head_offset=HEAD_OFFSET, n_param=N_PARAM,
                 lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, apply_adam=1, any_clip=0, slabs_per_graph=0, stream=None)
        return v


def call(api, entry, alter):
    """the return code of ``drgnn_<entry>`` for the valid call with ``alter`` applied: argument name -> value,
    ``optim.<member>`` / ``optim.<member>[i]`` -> value, ``zero_ptr[i]`` / ``zero_len[i]`` -> value"""
    w = World()
    v = w.values()
    for key, val in alter.items():
        m = re.match(r"^(optim\.)?(\w+?)(?:\[(\d+)\])?$", key)
        record, name, idx = m.group(1), m.group(2), m.group(3)
        if record or idx is not None:
            target = w.optim if record else w
            if idx is None:
                setattr(target, name, val)
            else:
                getattr(target, name)[int(idx)] = val
        else:
            assert key in SIGS[entry], (entry, key)
            v[key] = val
    return int(getattr(api.lib, "drgnn_" + entry)(*[v[name] for name in SIGS[entry]]))


PLAIN = ("train_update", "step_update")
OPT = ("train_update_opt", "step_update_opt")
STEP = ("step_update", "step_update_opt")
COHORT = ("cohort_update", "cohort_update_opt")
CLIP = {"optim.clip": 1}

# (entry, what, the valid call the case starts from, the one alteration, code -- or {"emu": code, "hip": code})
REFUSALS = []
# (entry, what, alteration of the first valid call, code): calls the emulation build carries out
VALID = []


def _refuse(entry, what, alter, code, base=None):
    REFUSALS.append((entry, what, dict(base or {}), alter, code))


for e in PLAIN + OPT:
    VALID.append((e, "valid", {}, 0))
    for name in ("net", "conv_partials", "head_partials", "flat_grad", "g_conv1", "g_conv2"):
        _refuse(e, "null " + name, {name: None}, E_ARG)
    for name in ("flat_param", "exp_avg", "exp_avg_sq", "step"):
        _refuse(e, "adam with null " + name, {name: None}, E_ARG)
        if name != "step" or e not in STEP:
            VALID.append((e, "no adam, null " + name, {"apply_adam": 0, name: None}, 0))
    VALID.append((e, "no adam", {"apply_adam": 0}, 0))
for e in STEP:
    _refuse(e, "null readout", {"readout": None}, E_ARG)
    _refuse(e, "no adam, null step2", {"step": None}, E_ARG, base={"apply_adam": 0})
for e in STEP + ("step_gradients",):
    for s in (-1, 3):
        _refuse(e, "slabs_per_graph %d" % s, {"slabs_per_graph": s}, E_ARG)
    for s in (1, 2):
        VALID.append((e, "slabs_per_graph %d" % s, {"slabs_per_graph": s}, 0))
for e in OPT:
    VALID.append((e, "valid, clipping", CLIP, 0))
    _refuse(e, "null optim", {"optim": None}, E_ARG)
    _refuse(e, "lr_n negative", {"optim.lr_n": -1}, E_ARG)
    _refuse(e, "lr_n without table", {"optim.lr_n": 1}, E_ARG)
    _refuse(e, "n_dead negative", {"optim.n_dead": -1}, E_ARG)
    _refuse(e, "n_dead too large", {"optim.n_dead": ZERO_RANGES + 1}, E_ARG)
    _refuse(e, "dead_off negative", {"optim.dead_off[0]": -1}, E_ARG)
    _refuse(e, "dead_len negative", {"optim.dead_len[0]": -1}, E_ARG)
    _refuse(e, "clip, null norm_words", {"optim.norm_words": None}, E_ARG, base=CLIP)
    _refuse(e, "clip, norm_cap 0", {"optim.norm_cap": 0}, E_ARG, base=CLIP)
    # (the product: more update blocks than words; the emulation: more flat 256-element words than words)
    _refuse(e, "clip, norm_cap 1", {"optim.norm_cap": 1}, E_CAPACITY, base=CLIP)
for e in COHORT:
    VALID.append((e, "valid", {}, E_CAPACITY))          # (the emulation build has no cohort launches)
    _refuse(e, "null members", {"members": None}, E_ARG)
    _refuse(e, "K 0", {"K": 0}, E_ARG)
    _refuse(e, "K 65536", {"K": 65536}, E_ARG)
    _refuse(e, "null counts", {"counts": None}, E_ARG)
    _refuse(e, "n_param 0", {"n_param": 0}, E_ARG)
    _refuse(e, "head_offset negative", {"head_offset": -1}, E_ARG)
    _refuse(e, "head_offset n_param", {"head_offset": N_PARAM}, E_ARG)
    _refuse(e, "null net", {"net": None}, E_WIDTH)
    _refuse(e, "null g_conv1", {"g_conv1": None}, E_ARG)
    _refuse(e, "null g_conv2", {"g_conv2": None}, E_ARG)
_refuse("cohort_update_opt", "null optims", {"optims": None}, E_ARG)
for e in COHORT + ("step_gradients",):
    _refuse(e, "R not 32 per branch", {"R": R + 1}, E_WIDTH)
    _refuse(e, "H 0", {"H": 0}, E_WIDTH)
    _refuse(e, "H 513", {"H": 513}, E_WIDTH)
    _refuse(e, "O 0", {"O": 0}, E_WIDTH)
    _refuse(e, "O too large", {"O": MAX_OUT + 1}, E_WIDTH)
VALID.append(("step_gradients", "valid", {}, 0))
VALID.append(("step_gradients", "no weights, no step word, nothing to clear", {"graph_weight": None, "step": None, "n_zero": 0}, 0))
for name in ("net", "conv_partials", "g_conv1", "g_conv2", "head_partials", "readout", "head_grad"):
    _refuse("step_gradients", "null " + name, {name: None}, E_ARG)
_refuse("step_gradients", "n_graphs negative", {"n_graphs": -1}, E_ARG)
_refuse("step_gradients", "n_zero negative", {"n_zero": -1}, E_ARG)
_refuse("step_gradients", "n_zero too large", {"n_zero": ZERO_RANGES + 1}, E_ARG)
_refuse("step_gradients", "null zero_ptr", {"zero_ptr": None}, E_ARG)
_refuse("step_gradients", "null zero_len", {"zero_len": None}, E_ARG)
_refuse("step_gradients", "null range", {"zero_ptr[0]": None}, E_ARG)
_refuse("step_gradients", "negative range", {"zero_len[0]": -1}, E_ARG)
VALID.append(("net_reduce_grads", "valid", {}, 0))
for name in ("net", "conv_partials", "g_conv1", "g_conv2"):
    _refuse("net_reduce_grads", "null " + name, {name: None}, E_ARG)


def case_id(case):
    return "%s-%s" % (case[0], case[1].replace(" ", "_").replace(",", ""))


def check_refusal(api, build, case):
    entry, what, base, alter, code = case
    both = dict(base)
    both.update(alter)
    assert call(api, entry, both) == (code[build] if isinstance(code, dict) else code), (entry, what)


def check_valid(api, case):
    entry, what, alter, code = case
    assert call(api, entry, alter) == code, (entry, what)
