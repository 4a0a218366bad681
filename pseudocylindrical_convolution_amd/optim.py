"""The optimiser step on this project's arithmetic, and the whole state of a training run in one file.

`Adam` is torch.optim.Adam's update (no weight decay, no amsgrad) as include/pconv_hip.h defines it operation by
operation ("THE ORDER of the optimiser step"): the step gradient g = acc + grad, its global norm as a two-stage fp64
sum of fixed shape (segments of 4096 elements, 256 lanes, a fixed tree), clip_grad_norm_'s coefficient, and the
element-wise update in fp32 with every operation rounded on its own.  On GPU tensors that is three launches of
csrc/optim.hip (PCONV.optim_sqnorm, PCONV.optim_adam) over a device table of the tensors; on CPU tensors `_twin`
below restates the same operations, the 256-lane shape and the tree included, and gives the same bits (the
erp_resample pattern: `--device cpu --optim native` works, and the CPU and GPU tests share their cases).  The state
layout is torch.optim.Adam's, so either optimiser's state_dict() loads into the other.

`TrainState` saves and restores everything the trajectory of train.py depends on: model, optimisers, position in the
epoch, gradient accumulators, the quantiser ops' call counters, the best losses, the sampler's seed extension, the
random generators, the history, and a fingerprint of the arguments that shape the run.
"""
import math
import os

import numpy as np
import torch

from .PCONV_operator import backend

SEGMENT = 4096   # elements per segment
LANES = 256      # lanes per segment; a lane takes quads l, l + 256, ...
QUAD = 4


# ---- the CPU twin of csrc/optim.hip -------------------------------------------------------------------------------

def _tree(a):
    """for s = 128 ... 1: a[l] += a[l + s] for l < s, on the last axis of `a` (LANES wide); returns a[..., 0]"""
    s = LANES // 2
    while s >= 1:
        a[..., :s] = a[..., :s] + a[..., s:2 * s]
        s //= 2
    return a[..., 0]


def _lane_sum(values, per_lane):
    """values (rows, k * LANES * per_lane) fp64, zero padded: lane l adds its items of round 0, round 1, ... in
    ascending order from +0 (adding a padding +0 changes no bit: every sum here is of squares or of such sums), then
    the tree"""
    rows = values.shape[0]
    v = values.reshape(rows, -1, LANES, per_lane)
    a = np.zeros((rows, LANES), dtype=np.float64)
    for r in range(v.shape[1]):
        for e in range(per_lane):
            a = a + v[:, r, :, e]
    return _tree(a)


def _padded(x, multiple):
    n = -(-x.size // multiple) * multiple
    out = np.zeros(max(n, multiple), dtype=x.dtype)
    out[:x.size] = x
    return out


def _twin_sqnorm(items, clip):
    """(total, norm fp64, coef fp32) of the step gradients of `items`, in THE ORDER"""
    partials = []
    for it in items:
        g = it["grad"] if it["acc"] is None else it["acc"] + it["grad"]
        g = g.astype(np.float64)
        partials.append(_lane_sum(_padded(g * g, SEGMENT).reshape(-1, SEGMENT), QUAD))
    total = _lane_sum(_padded(np.concatenate(partials), LANES).reshape(1, -1), 1)[0]
    norm = np.sqrt(total)
    coef = np.float64(1.0)
    if clip > 0:
        c = np.float64(np.float32(clip)) / (norm + np.float64(1e-6))
        coef = c if c < 1.0 else (c if c != c else np.float64(1.0))   # min(1, c) that keeps a NaN
    return total, norm, np.float32(coef)


def _twin(items, clip):
    """the step of csrc/optim.hip on flat float32 numpy views, in place; returns (total, norm, coef)"""
    with np.errstate(all="ignore"):
        total, norm, coef = _twin_sqnorm(items, clip)
        for it in items:
            p, m, v = it["p"], it["m"], it["v"]
            step_size, bc2_sqrt, eps, omb1, beta2, omb2 = it["scalars"]
            g = it["grad"] if it["acc"] is None else it["acc"] + it["grad"]
            g = g * coef
            m[...] = m + omb1 * (g - m)
            v[...] = (beta2 * v) + omb2 * (g * g)
            den = np.sqrt(v) / bc2_sqrt + eps
            p[...] = p - step_size * (m / den)
            if it["acc"] is not None:
                it["acc"][...] = 0.0
    return total, norm, coef


def _scalars(lr, beta1, beta2, eps, t):
    """(step_size, bc2_sqrt, eps, 1 - beta1, beta2, 1 - beta2): computed in fp64, each rounded once to fp32"""
    return tuple(np.float32(x) for x in (lr / (1.0 - beta1 ** t), math.sqrt(1.0 - beta2 ** t), eps, 1.0 - beta1, beta2,
                                         1.0 - beta2))


class Adam(torch.optim.Optimizer):
    """torch.optim.Adam(params, lr, betas, eps) with the step of include/pconv_hip.h.  step(acc=, clip=) takes the
    gradient accumulators (AccGrad.acc_grad, aligned with the parameters) and the global norm bound, so that it
    stands for AccGrad.copy_back + clip_grad_norm_ + Adam.step; afterwards `last_grad_norm` is the norm of the step
    gradient as a 0-dim fp64 tensor on the parameters' device (nothing is synchronised), `last_total` its square and
    `last_coef` (fp32) the clip coefficient that was applied."""

    REFUSED = ("weight_decay", "amsgrad", "maximize")

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, **unsupported):
        for name, value in unsupported.items():
            if name not in self.REFUSED:
                raise TypeError("optim.Adam: unexpected argument %r" % name)
            if value:
                raise ValueError("optim.Adam: %s=%r is not supported (plain Adam only)" % (name, value))
        if not (lr >= 0 and eps >= 0 and 0 <= betas[0] < 1 and 0 <= betas[1] < 1):
            raise ValueError("optim.Adam: bad lr %r, betas %r or eps %r" % (lr, betas, eps))
        # every key of torch.optim.Adam's groups, so that a state_dict() of this class loads into that one
        defaults = dict(torch.optim.Adam([torch.zeros(1)], lr=lr, betas=betas, eps=eps).defaults)
        super(Adam, self).__init__(params, defaults)
        self.last_grad_norm = self.last_total = self.last_coef = None
        self._segments = {}

    def _plan(self, acc):
        """the tensors that take part, checked: [(group, p, acc or None)]; refuses by name before any state changes"""
        params = [(g, p) for g in self.param_groups for p in g["params"]]
        if acc is not None and len(acc) != len(params):
            raise ValueError("optim.Adam: %d accumulators for %d parameters" % (len(acc), len(params)))
        for gi, g in enumerate(self.param_groups):
            for name in self.REFUSED:
                if g.get(name):
                    raise ValueError("optim.Adam: group %d has %s=%r, which is not supported" % (gi, name, g[name]))
        plan, device = [], None
        for i, (g, p) in enumerate(params):
            if p.grad is None:
                continue
            a = None if acc is None else acc[i]
            state = self.state.get(p, {})
            for what, t in (("parameter", p), ("gradient", p.grad), ("accumulator", a),
                            ("exp_avg", state.get("exp_avg")), ("exp_avg_sq", state.get("exp_avg_sq"))):
                if t is None:
                    continue
                where = "optim.Adam: %s %d (shape %s)" % (what, i, tuple(t.shape))
                if t.is_sparse or t.layout != torch.strided or not t.is_contiguous():
                    raise ValueError("%s is not dense" % where)
                if t.dtype != torch.float32:
                    raise ValueError("%s is %s, not float32" % (where, t.dtype))
                if t.shape != p.shape:
                    raise ValueError("%s does not have the parameter's shape %s" % (where, tuple(p.shape)))
                device = t.device if device is None else device
                if t.device != device:
                    raise ValueError("%s is on %s, the others on %s" % (where, t.device, device))
            plan.append((g, p, a))
        return plan, device

    @torch.no_grad()
    def step(self, closure=None, acc=None, clip=0.0):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        plan, device = self._plan(acc)
        clip = float(clip)
        items = []
        for g, p, a in plan:
            state = self.state[p]
            if len(state) == 0:
                state["step"] = torch.tensor(0.0, dtype=torch.float32)
                state["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                state["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            state["step"] += 1
            if p.numel():
                items.append((p, p.grad, a, state["exp_avg"], state["exp_avg_sq"],
                              _scalars(g["lr"], g["betas"][0], g["betas"][1], g["eps"], float(state["step"]))))
        if not items:
            return loss
        if device.type == "cuda":
            total, norm, coef = self._step_gpu(items, clip, device)
        else:
            flat = lambda t: None if t is None else t.detach().view(-1).numpy()
            total, norm, coef = (torch.from_numpy(np.asarray(x).reshape(())) for x in _twin(
                [dict(p=flat(p), grad=flat(gr), acc=flat(a), m=flat(m), v=flat(v), scalars=s)
                 for p, gr, a, m, v, s in items], clip))
        # written through raw pointers: tell autograd, and whoever keys a cache on a parameter's version (the packed
        # weights of the convolutions, PCONV._cached_pack), that the tensors changed in place
        torch.autograd.graph.increment_version([t for p, _, a, m, v, _ in items for t in (p, a, m, v) if t is not None])
        self.last_total, self.last_grad_norm, self.last_coef = total, norm, coef
        return loss

    def _step_gpu(self, items, clip, device):
        ops = backend.ops()
        if not hasattr(ops, "optim_step"):
            raise RuntimeError("optim.Adam: the active backend has no optimiser kernels for GPU tensors")
        records, segments = self._tables(ops, items, device)
        ws = ops.optim_step(records, segments, clip, device)
        return ws[0], ws[1], ws[2:3].view(torch.float32)[0]

    def _tables(self, ops, items, device):
        """(the device table of pconv_optim_tensor records of `items`, their segment table)"""
        counts = tuple(p.numel() for p, _, _, _, _, _ in items)
        key = (counts, device)
        if key not in self._segments:   # sizes only: built once
            self._segments = {key: ops.optim_segments(counts, device)}
        ints = np.array([[p.data_ptr(), gr.data_ptr(), 0 if a is None else a.data_ptr(), m.data_ptr(), v.data_ptr(),
                          p.numel()] for p, gr, a, m, v, _ in items], dtype=np.int64)
        floats = np.array([s for _, _, _, _, _, s in items], dtype=np.float32)
        # the pointers (new gradients after every zero_grad()) and the bias corrections change with every step; a
        # pageable host array is staged by the runtime before .to() returns, so it may be dropped at once
        return torch.from_numpy(np.concatenate([ints, floats.view(np.int64)], axis=1)).to(device), self._segments[key]


# ---- the state of a training run ------------------------------------------------------------------------------------

def rng_get(device):
    return {"cpu": torch.get_rng_state(), "device": torch.cuda.get_rng_state(device) if device.type == "cuda" else None}


def rng_set(state, device):
    torch.set_rng_state(state["cpu"])
    if state["device"] is not None and device.type == "cuda":
        torch.cuda.set_rng_state(state["device"], device)


def _quantisers(model):
    return {name: m for name, m in model.named_modules() if hasattr(m, "call_counters")}


class TrainState(object):
    """Where a run of train.py stands, and save / load of everything its trajectory depends on.

    epoch, next_batch: the batch (index in the epoch's loader order) the run trains next; global_batch: batches
    trained so far; acc: the gradient accumulators where next_batch falls inside an accumulation window; last: the
    loss figures of the last trained batch; history: the Job's history over the finished epochs; rng_epoch: the
    random generators as the epoch in flight found them (the loader's iterator is made from that state again)."""

    # the arguments that do not shape the trajectory: a resumed run may change them
    FREE = ("epochs", "time_budget", "stop_after", "resume", "verbose", "workers", "base_dir")
    DERIVED = ("deadline", "gpu_id")   # what train.py itself hangs on the namespace
    LATER = ("vp_size", "code_size", "cube_kind", "cube_face")   # arguments newer than the first state files: at their default (None) they leave no trace

    def __init__(self):
        self.epoch, self.next_batch, self.global_batch = 1, 0, 0
        self.acc = self.last = self.rng_epoch = self.rng = None
        self.history = []
        self.world_size, self.stopped = 1, False   # of the process, not of the file: ranks, and "stopped early"

    @classmethod
    def fingerprint(cls, args, world_size):
        fp = {k: v for k, v in sorted(vars(args).items()) if k not in cls.FREE and k not in cls.DERIVED
              and not (k in cls.LATER and v is None)}
        fp["world_size"] = int(world_size)
        return fp

    def save(self, path, args, world_size, model, optimizers, saver, sampler, device):
        """write the state file: under a temporary name first, then os.replace -- a file cut short never stands under
        `path`.  model: the bare module; optimizers: {name: optimiser or None}; called by rank 0"""
        blob = {
            "fingerprint": self.fingerprint(args, world_size),
            "model": model.state_dict(),
            "optimizers": {k: o.state_dict() for k, o in optimizers.items() if o is not None},
            "epoch": self.epoch, "next_batch": self.next_batch, "global_batch": self.global_batch,
            "acc": None if self.acc is None else [a.detach().cpu() for a in self.acc],
            "last": self.last, "history": [[list(last) if last is not None else None, list(ls)] for last, ls in self.history],
            "quant_calls": {name: q.call_counters() for name, q in _quantisers(model).items()},
            "saver": None if saver is None else {"current_best_loss": saver.current_best_loss, "init": saver.init},
            "seed_ext": sampler.seed_ext,
            "rng": rng_get(device), "rng_epoch": self.rng_epoch,
        }
        tmp = "%s.tmp.%d" % (path, os.getpid())
        try:
            torch.save(blob, tmp)
            os.replace(tmp, path)
        finally:
            if os.path.exists(tmp):
                os.remove(tmp)

    @classmethod
    def load(cls, path, args, world_size, model, optimizers, saver, sampler, device):
        """restore everything `save` wrote into the objects given and return the TrainState; refuses a file written
        under other trajectory-shaping arguments, naming the first that differs.  Every rank reads the file."""
        if not os.path.exists(path):
            raise FileNotFoundError("--resume: no training state at %s (a run without --resume starts afresh)" % path)
        blob = torch.load(path, map_location="cpu")
        now = cls.fingerprint(args, world_size)
        for k in sorted(set(now) | set(blob["fingerprint"])):
            if k not in now or k not in blob["fingerprint"] or now[k] != blob["fingerprint"][k]:
                shown = "world size" if k == "world_size" else "--" + k.replace("_", "-")
                raise ValueError("--resume: {} was written with {} = {!r}, this run has {!r}: the run would not continue "
                                 "the one that stopped".format(path, shown, blob["fingerprint"].get(k), now.get(k)))
        model.load_state_dict(blob["model"])
        for k, o in optimizers.items():
            if o is not None:
                o.load_state_dict(blob["optimizers"][k])
        for name, q in _quantisers(model).items():
            q.set_call_counters(blob["quant_calls"][name])
        if saver is not None and blob["saver"] is not None:
            saver.current_best_loss, saver.init = blob["saver"]["current_best_loss"], blob["saver"]["init"]
        sampler.seed_ext = blob["seed_ext"]
        rng_set(blob["rng"], device)
        st = cls()
        st.epoch, st.next_batch, st.global_batch = blob["epoch"], blob["next_batch"], blob["global_batch"]
        st.acc = None if blob["acc"] is None else [a.to(device) for a in blob["acc"]]
        st.last = None if blob["last"] is None else tuple(blob["last"])
        st.history = [(None if last is None else tuple(last), ls) for last, ls in blob["history"]]
        st.rng_epoch, st.rng = blob["rng_epoch"], blob["rng"]
        return st
