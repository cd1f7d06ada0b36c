"""The last third of the reference's training step — `optimizer.step()`, `ema.update(model_train)`, and the learning rate `set_optimizer_lr` writes once per epoch
(utils/utils_fit.py:117-118,164-174, loss/detection_loss.py:433-459,488-526, train.py:499-523) — as TWO launches over one flat arena (csrc/k_optim.h), whatever the
number of tensors.  The reference issues two small kernels for every floating state-dict entry in `ModelEMA.update` alone.

`FusedOptimizer` re-points the model's parameters and float buffers into an fp32 arena it allocates (`t.data = view`: the tensors stay the objects they were, with
their values), keeps gradient, momentum and EMA arenas of the same layout, and updates all of them with `ach_optim_tick` + `ach_optim_step`.  Every address the kernels
see lies inside an arena allocated here and every index is a chunk number below a count derived from that arena's `numel()`; no pointer is collected from autograd.
The EMA is a servable module: `opt.ema_model` is a deep copy of the model in `.eval()` whose float tensors alias the EMA arena.

The learning rate and weight decay live in a small device array (`hyper`), written by the host when `param_groups[g]['lr']` changes: a captured step
(train_graph.GraphedTrainStep) reads it on every replay.  GPU tensors only; there is no PyTorch-op fallback.
"""
import copy
import math

import torch

from . import _native as N

CHUNK = 256                                     # elements per chunk (csrc/k_optim.h OPT_CHUNK): every tensor's slot starts at a multiple of it
KINDS = {'sgd': 0, 'adam': 1, 'adamw': 2}
FLAG_FROZEN, FLAG_BUFFER, FLAG_ACTIVE = 3, 4, 8
H_LR, H_WD, H_DECAY, H_TAU, H_UPDATES, H_D, H_LEN = 0, 3, 6, 7, 8, 9, 10       # k_optim.h OPT_*


def reference_param_groups(model):
    """The reference's grouping (train.py:499-513) restated on names and buffers, as parameter NAMES: `(pg0, pg1, pg2, ungrouped)`.
    pg0: the weight of every BatchNorm2d — here a node that owns `running_mean` — or of any module whose path contains "bn" (no decay); pg1: every other `.weight`
    (weight_decay); pg2: every `.bias`; `ungrouped`: the parameters the reference never hands to its optimizer (gamma, gamma_xca, temperature, cweight, cbias, sweight,
    sbias).  backbone 'rv' (train.py:514-518): ONE group holding all parameters."""
    names = {id(p): k for k, p in model.named_parameters()}
    if getattr(model, 'backbone', None) == 'rv':
        return list(names.values()), [], [], []
    pg0, pg1, pg2 = [], [], []
    for k, v in model.named_modules():
        bias, weight = v._parameters.get('bias'), v._parameters.get('weight')
        if bias is not None:
            pg2.append(names[id(bias)])
        if 'running_mean' in v._buffers or 'bn' in k:
            if weight is not None:
                pg0.append(names[id(weight)])
        elif weight is not None:
            pg1.append(names[id(weight)])
    taken = set(pg0) | set(pg1) | set(pg2)
    return pg0, pg1, pg2, [k for k in names.values() if k not in taken]


def _slots(tensors, first_chunk):
    """[(first chunk, chunks)] of tensors laid out one behind the other, each from a chunk boundary"""
    out = []
    for t in tensors:
        n = max(1, -(-t.numel() // CHUNK))
        out.append((first_chunk, n))
        first_chunk += n
    return out, first_chunk


class FusedOptimizer(torch.optim.Optimizer):
    """SGD (momentum, Nesterov), Adam or AdamW over up to three parameter groups, plus the reference's `ModelEMA`, in two launches a step.

        opt = FusedOptimizer(model, 'sgd', lr, momentum=0.937, weight_decay=5e-4)        # groups='reference': train.py's pg0 / pg1 / pg2
        ...
        loss.backward(); opt.step(); opt.zero_grad()                                      # step() = optimizer.step() + ema.update(model)
        set_optimizer_lr(opt, lr_scheduler_func, epoch)                                   # the reference's, unchanged
        opt.ema_model(x, radar, points)                                                   # the averaged weights, served

    `groups`: 'reference', or a list of torch-style dicts ({'params': [...], 'lr': ..., 'weight_decay': ...}), at most three; a parameter of the model in no group is never
    optimised (its EMA still follows it).  For the reference's 'rv' form pass momentum=0 (plain SGD) or kind='adamw'.  `ema_updates`: ModelEMA's `updates` to resume from.
    After construction the model's parameters and float buffers ALIAS the arena `state`: `.to()`, `.cuda()` or `load_state_dict(assign=True)` break that and `step()`
    raises; an in-place `load_state_dict` is fine.  `optimizer.state` stays empty: the arenas are `graph_state()` / `state_dict()`."""

    def __init__(self, model, kind='sgd', lr=1e-2, momentum=0.937, nesterov=True, betas=(0.937, 0.999), eps=1e-8, weight_decay=5e-4, groups='reference',
                 ema=True, ema_decay=0.9999, ema_tau=2000, ema_updates=0):
        if kind not in KINDS:
            raise ValueError(f"FusedOptimizer: kind must be 'sgd', 'adam' or 'adamw', got {kind!r}")
        named = dict(model.named_parameters())
        if groups == 'reference':
            pg0, pg1, pg2, _ = reference_param_groups(model)
            if getattr(model, 'backbone', None) == 'rv':
                groups = [{'params': [named[k] for k in pg0], 'weight_decay': weight_decay}]
            else:
                groups = [{'params': [named[k] for k in pg0], 'weight_decay': 0.0}, {'params': [named[k] for k in pg1], 'weight_decay': weight_decay},
                          {'params': [named[k] for k in pg2], 'weight_decay': 0.0}]
        groups = [dict(g, params=list(g['params'])) for g in groups]
        if not 1 <= len(groups) <= 3:
            raise ValueError(f"FusedOptimizer: one to three parameter groups, got {len(groups)}")
        of_model = {id(p) for p in named.values()}
        grouped = [p for g in groups for p in g['params']]
        if len({id(p) for p in grouped}) != len(grouped) or any(id(p) not in of_model for p in grouped):
            raise ValueError("FusedOptimizer: every grouped parameter must be a parameter of `model`, in one group")
        taken = {id(p) for p in grouped}
        frozen = [p for p in named.values() if id(p) not in taken]
        buffers = [b for b in model.buffers() if b.is_floating_point()]
        tensors = grouped + frozen + buffers
        if not tensors or any(t.dtype != torch.float32 for t in tensors):
            raise TypeError("FusedOptimizer: the arenas are float32; every parameter and float buffer of the model must be")
        dev = tensors[0].device
        if any(t.device != dev for t in tensors):
            raise ValueError("FusedOptimizer: the model's tensors are on more than one device")
        self.kind, self.momentum, self.nesterov, self.betas, self.eps = kind, float(momentum), bool(nesterov), (float(betas[0]), float(betas[1])), float(eps)
        self._lib = N.lib(tensors[0])                                      # raises for CPU tensors: there is no CPU path
        self.device = dev
        ema_model = copy.deepcopy(model).eval().requires_grad_(False) if ema else None       # (before the model aliases an arena: a copy of a view copies its whole storage)

        # ---- layout: [group 0 | group 1 | group 2 | parameters in no group | float buffers], every slot from a chunk boundary
        slots, self.param_chunks = _slots(grouped + frozen, 0)
        bslots, self.chunks = _slots(buffers, self.param_chunks)
        slots += bslots
        self._tensors, self._slots, self._n_opt = tensors, slots, len(grouped)
        z = dict(dtype=torch.float32, device=dev)
        self.state_arena = torch.zeros(self.chunks * CHUNK, **z)
        self.grad_arena = torch.zeros(self.param_chunks * CHUNK, **z)
        self.m1 = torch.zeros(self.param_chunks * CHUNK, **z) if (kind != 'sgd' or self.momentum != 0.0) else None
        self.m2 = torch.zeros(self.param_chunks * CHUNK, **z) if kind != 'sgd' else None
        self.t = torch.zeros(self.param_chunks, dtype=torch.int32, device=dev) if kind != 'sgd' else None
        self.ema_arena = torch.zeros(self.chunks * CHUNK, **z) if ema else None
        with torch.no_grad():
            for t, view in zip(tensors, self._views(self.state_arena, tensors)):
                view.copy_(t)
                t.data = view
        self._owners = self._owners_of(model, tensors)
        self._ptrs = [t.data_ptr() for t in tensors]
        self._grad_views = self._views(self.grad_arena, grouped)
        self.ema_model = ema_model
        self._ema_tensors = []
        if ema:
            e_named, e_bufs = dict(ema_model.named_parameters()), dict(ema_model.named_buffers())
            of = {id(p): e_named[k] for k, p in named.items()}
            of.update({id(b): e_bufs[k] for k, b in model.named_buffers()})
            self._ema_tensors = [of[id(t)] for t in tensors]
            with torch.no_grad():
                for t, view in zip(self._ema_tensors, self._views(self.ema_arena, tensors)):
                    view.copy_(t)
                    t.data = view
            self._ema_owners = self._owners_of(ema_model, self._ema_tensors)
            self._ema_ptrs = [t.data_ptr() for t in self._ema_tensors]

        # ---- per-chunk flags: the group id, 3 = never optimised, 4 = a float buffer; bit 3 = the parameter has a gradient this step
        base = torch.full((self.chunks,), FLAG_BUFFER, dtype=torch.int32)
        gid = [g for g, grp in enumerate(groups) for _ in grp['params']] + [FLAG_FROZEN] * len(frozen)
        for (a, n), g in zip(slots, gid):
            base[a:a + n] = g
        self._flags_base = base
        self._flags_host = self._host(torch.int32, self.chunks)
        self.flags = torch.zeros(self.chunks, dtype=torch.int32, device=dev)
        self._inactive = None                                              # the cached set: (parameter i has no gradient) for the optimised parameters
        self._hyper_host = self._host(torch.float64, H_LEN)
        self.hyper = torch.zeros(H_LEN, dtype=torch.float64, device=dev)
        self._uploaded = None                                              # event behind the last copy out of a pinned host tensor

        super().__init__(groups, dict(lr=float(lr), weight_decay=0.0))
        self.use_ema = bool(ema)
        h = self._hyper_host
        h.zero_()
        h[H_DECAY], h[H_TAU], h[H_UPDATES] = float(ema_decay), float(ema_tau), float(ema_updates)
        h[H_D] = float(ema_decay) * (1 - math.exp(-float(ema_updates) / float(ema_tau)))
        self._hyper_cached = self._group_values()
        h[:2 * 3] = torch.tensor(self._hyper_cached, dtype=torch.float64)
        self._upload(self.hyper, h)
        self._set_flags(tuple(False for _ in grouped))

    # ------------------------------------------------------------------------------------------------------------------ host side
    def _views(self, arena, tensors):
        return [arena[a * CHUNK:a * CHUNK + t.numel()].view(t.shape) for t, (a, _) in zip(tensors, self._slots)]

    def _host(self, dtype, n):
        t = torch.zeros(n, dtype=dtype)
        return t.pin_memory() if self.device.type == 'cuda' else t

    def _upload(self, dst, src):
        """dst <- the pinned host tensor src, asynchronously; `_host_ready()` before src is written again"""
        dst.copy_(src, non_blocking=True)
        if self.device.type == 'cuda':
            self._uploaded = torch.cuda.Event()
            self._uploaded.record(torch.cuda.current_stream(self.device))

    def _host_ready(self):
        if self._uploaded is not None:
            self._uploaded.synchronize()
            self._uploaded = None

    def _capturing(self):
        return self.device.type == 'cuda' and torch.cuda.is_current_stream_capturing()

    def _group_values(self):
        lr = [float(g['lr']) for g in self.param_groups] + [0.0] * (3 - len(self.param_groups))
        wd = [float(g['weight_decay']) for g in self.param_groups] + [0.0] * (3 - len(self.param_groups))
        return lr + wd

    def _set_flags(self, inactive):
        if self._capturing():
            raise RuntimeError("FusedOptimizer: the set of parameters without a gradient changed inside a stream capture (it is fixed when the step is captured)")
        self._host_ready()
        f = self._flags_host
        f.copy_(self._flags_base)
        for (a, n), off in zip(self._slots, inactive):
            if not off:
                f[a:a + n] += FLAG_ACTIVE
        self._upload(self.flags, f)
        self._inactive = inactive

    @staticmethod
    def _owners_of(module, tensors):
        """[(the `_parameters` / `_buffers` table that holds the tensor, its name there)]: where the module must still hold this very object"""
        at = {}
        for m in module.modules():
            for table in (m._parameters, m._buffers):
                for leaf, t in table.items():
                    if t is not None:
                        at.setdefault(id(t), (table, leaf))
        return [at[id(t)] for t in tensors]

    @staticmethod
    def _aliased(tensors, owners, ptrs):
        return all(table.get(leaf) is t and t.data_ptr() == ptr for t, (table, leaf), ptr in zip(tensors, owners, ptrs))

    def _check_aliasing(self):
        """the module still holds the tensor objects this optimizer re-pointed (load_state_dict(assign=True) and a moved buffer replace them) at the addresses it
        gave them (.to() / .cuda() move a parameter's data): host-only, ~0.1 ms"""
        if not self._aliased(self._tensors, self._owners, self._ptrs) or (self.use_ema and not self._aliased(self._ema_tensors, self._ema_owners, self._ema_ptrs)):
            raise RuntimeError("FusedOptimizer: a parameter or buffer no longer aliases its slot of the arena (after .to() / .cuda() / load_state_dict(assign=True)); "
                               "rebuild the optimizer on the model as it is now")

    def sync_hyperparameters(self):
        """param_groups[g]['lr'] / ['weight_decay'] -> `hyper`, if they changed: one small asynchronous copy.  (Also the host-only aliasing check of `step()`.)"""
        self._check_aliasing()
        now = self._group_values()
        if now != self._hyper_cached:
            if self._capturing():
                raise RuntimeError("FusedOptimizer: a learning rate or weight decay changed inside a stream capture; set it before the capture or between replays")
            self._host_ready()
            self._hyper_host[:6] = torch.tensor(now, dtype=torch.float64)
            self._upload(self.hyper[:6], self._hyper_host[:6])
            self._hyper_cached = now

    def set_lr(self, lr):
        for g in self.param_groups:
            g['lr'] = float(lr)

    def set_ema_updates(self, updates):
        """the reference's `ema.updates = epoch_step * epoch` (train.py:534-535, 671-672): the count the next step's tick continues from"""
        self._host_ready()
        self._hyper_host[H_UPDATES] = float(updates)
        self._upload(self.hyper[H_UPDATES:H_UPDATES + 1], self._hyper_host[H_UPDATES:H_UPDATES + 1])

    def mark_updated(self, everything=False):
        """bump the version counters of what a step writes through raw pointers — the optimised parameters, the EMA's parameters and buffers; `everything`: all of the
        model's tensors too (a loaded checkpoint) — so that `eval()` on either module re-folds its weights (nets.Achelous._weights_version)"""
        torch.autograd.graph.increment_version((self._tensors if everything else self._tensors[:self._n_opt]) + self._ema_tensors)

    def graph_state(self):
        """the tensors, besides the model's own, that a step writes: what train_graph.GraphedTrainStep snapshots before its warm-up steps and restores after the capture"""
        return [t for t in (self.m1, self.m2, self.ema_arena, self.t, self.hyper, self.grad_arena) if t is not None]

    # ------------------------------------------------------------------------------------------------------------------ the step
    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        self.sync_hyperparameters()
        params = self._tensors[:self._n_opt]
        inactive = tuple(p.grad is None for p in params)
        if inactive != self._inactive:
            self._set_flags(inactive)
        if not all(inactive):
            torch._foreach_copy_([v for v, off in zip(self._grad_views, inactive) if not off], [p.grad for p in params if p.grad is not None])
        L, s = self._lib, N.stream(self.state_arena)
        if self.use_ema:
            N.check(L, L.lib.ach_optim_tick(N.ptr(self.hyper), s), what='ach_optim_tick')
        N.check(L, L.lib.ach_optim_step(N.ptr(self.state_arena), N.ptr(self.ema_arena), N.ptr(self.grad_arena), N.ptr(self.m1), N.ptr(self.m2), N.ptr(self.flags),
                                        N.ptr(self.t), N.ptr(self.hyper), self.chunks, self.param_chunks, KINDS[self.kind], int(self.nesterov), self.momentum,
                                        self.betas[0], self.betas[1], self.eps, s), {-1: ValueError}, what='ach_optim_step')
        self.mark_updated()
        return loss

    # ------------------------------------------------------------------------------------------------------------------ checkpoints
    def _arenas(self):
        return {'state': self.state_arena, 'ema': self.ema_arena, 'm1': self.m1, 'm2': self.m2, 't': self.t, 'hyper': self.hyper}

    def state_dict(self):
        """the arenas, `t` and `hyper` (clones), the layout they belong to and the groups' scalars"""
        return {'kind': self.kind, 'layout': [list(s) for s in self._slots], 'arenas': {k: v.detach().clone() for k, v in self._arenas().items() if v is not None},
                'param_groups': [{k: v for k, v in g.items() if k != 'params'} for g in self.param_groups]}

    @torch.no_grad()
    def load_state_dict(self, state_dict):
        mine = {k: v for k, v in self._arenas().items() if v is not None}
        if state_dict['kind'] != self.kind or [list(s) for s in self._slots] != [list(s) for s in state_dict['layout']] or set(state_dict['arenas']) != set(mine):
            raise ValueError("FusedOptimizer.load_state_dict: the checkpoint was written by an optimizer of another kind or layout")
        for k, v in mine.items():
            v.copy_(state_dict['arenas'][k])
        for g, saved in zip(self.param_groups, state_dict['param_groups']):
            g.update(saved)
        h = state_dict['arenas']['hyper'].cpu()
        self._hyper_cached = [float(x) for x in h[:6]]           # what `hyper` now holds; a group value that differs is written by the next step
        self.mark_updated(everything=True)
