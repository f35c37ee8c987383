"""FusedAdam / FusedSGD / FusedAdamW: ``torch.optim.Adam`` / ``torch.optim.SGD`` / ``torch.optim.AdamW`` semantics in one HIP kernel per
slab segment.

Reference call site: train_chaos.py:218-223 (Adam, lr 1e-4, L2-coupled weight decay 3e-4) and
train_chaos.py:313-315 (zero_grad / backward / step).  The class keeps the ``torch.optim.Optimizer`` protocol
(``param_groups[i]['lr']`` is what utils.poly_lr_decay writes, ``zero_grad()``, ``step()``, ``state_dict()``),
but the update runs over the model's flat slabs (pacingpseudo_amd.flat.FlatSlab): p, g, m, v are read once and
p, m, v written once, 28 B per parameter, instead of one foreach launch chain per tensor list.

Step counts live ON THE DEVICE (round 5): one int32 per slab segment, advanced by the library after an update
that really happened.  A step the 16-bit storage mode's overflow guard skipped therefore does not advance Adam's bias
corrections (``torch.cuda.amp.GradScaler.step`` does not count skipped steps either), is counted ONCE in ``flat.guard[1]``
however many segments the step had, and nothing the kernels read per step is a host value -- which is what lets a captured
hipGraph of the whole iteration replay correctly.  The learning rate is mirrored into a device scalar for the same reason
(``sync_hyper``: refreshed whenever ``param_groups[i]['lr']`` changed, i.e. once per epoch).

Gradient-norm clipping (``max_grad_norm``, off by default): ``torch.nn.utils.clip_grad_norm_(params, max_norm, norm_type=2)``
over the parameters that carry a gradient, with the norm and the coefficient as DEVICE scalars -- per slab one streaming
sum-of-squares launch per active segment (double accumulation, no atomics: bit-reproducible), one finalize launch, and the update
kernels multiply every gradient element by the coefficient as they load it.  One difference from torch: the gradient slab is NOT
scaled in place (a second 8 B / parameter pass for nothing) -- ``p.grad`` keeps the raw gradient after ``step()``.  ``step()`` runs
behind the all-reduce and behind ``unscale_grads``, so data-parallel ranks compute the same coefficient from the same averaged
slab without a collective, and 16-bit storage runs clip the unscaled gradients.

EMA of the weights (``ema_decay``, off by default): every slab the optimizer updates gets an fp32 shadow slab ``ema``, created with
the moments and initialised from the parameters, and the ``*_step_ema`` kernels move it towards the parameters they have just
computed: ``e += fl32(w * fl32(p - e))``, ``w = fl32(1 - min(D, (1 + t) / (10 + t)))`` with t the segment's device step count
before the update (``ema_warmup_weight``).  Nothing of it is a host value but D, so it replays from a hipGraph, respects the
overflow guard (a skipped step leaves the shadow and t alone) and travels with ``state_dict()``.  Training does not depend on it.
Slab ranges the optimizer never updated are not averaged.  ``ema_weights()`` swaps the average in for evaluation,
``ema_state_dict(model)`` reads the model as it stands then.
"""
from __future__ import annotations

import contextlib
import math

import torch

from ._lib import lib, prof_range, stream_ptr


def check_max_grad_norm(value):
    """``max_grad_norm`` as the optimizers store it: None (off) or a float > 0; +inf = measure the norm, never clip."""
    if value is None:
        return None
    value = float(value)
    if math.isnan(value) or value <= 0.0:
        raise ValueError(f'max_grad_norm must be None (off) or > 0 (inf: measure only), got {value!r}')
    return value


def check_ema_decay(value):
    """``ema_decay`` as the optimizers store it: None (off) or a float with 0 < D < 1."""
    if value is None:
        return None
    value = float(value)
    if math.isnan(value) or not 0.0 < value < 1.0:
        raise ValueError(f'ema_decay must be None (off) or lie strictly between 0 and 1, got {value!r}')
    return value


def ema_warmup_weight(t: int, decay: float) -> float:
    """The weight w of the update ``e += w * (p - e)`` that follows t earlier updates, as the kernels form it: d_t = min(D,
    (1 + t) / (10 + t)) in double, w = 1 - d_t rounded once to fp32 (returned as the python float of that fp32 value)."""
    t = float(int(t))
    return float(torch.tensor(1.0 - min(float(decay), (1.0 + t) / (10.0 + t)), dtype=torch.float64).to(torch.float32))


def _nonneg_float(text):
    import argparse
    v = float(text)
    if math.isnan(v) or v < 0.0:
        raise argparse.ArgumentTypeError(f'must be >= 0 (0 = off, inf = measure only), got {text!r}')
    return v


def add_clip_flag(parser) -> None:
    """``--clip_grad_norm X`` of both training drivers (0 = off; resume.py knows this default for state files older than the flag)."""
    parser.add_argument('--clip_grad_norm', type=_nonneg_float, default=0.0,
                        help='clip the global L2 norm of the gradients to this value before every optimizer step '
                             '(torch.nn.utils.clip_grad_norm_ semantics, computed on the device; p.grad itself is not scaled); '
                             'inf: only measure and log the norm; 0 = off')


def _decay_float(text):
    import argparse
    v = float(text)
    if math.isnan(v) or not 0.0 <= v < 1.0:
        raise argparse.ArgumentTypeError(f'must be 0 (off) or lie strictly between 0 and 1, got {text!r}')
    return v


def _positive_int(text):
    import argparse
    v = int(text)
    if v < 1:
        raise argparse.ArgumentTypeError(f'must be >= 1, got {text!r}')
    return v


positive_int = _positive_int          # the drivers' own flags use the same validators


def positive_float(text):
    import argparse
    v = float(text)
    if not (v > 0.0 and v < math.inf):
        raise argparse.ArgumentTypeError(f'must be a positive finite number, got {text!r}')
    return v


def add_ema_flags(parser) -> None:
    """``--ema_decay D`` / ``--ema_val_interval N`` of both training drivers (0 = off; resume.py knows the defaults for state files
    older than the flags)."""
    parser.add_argument('--ema_decay', type=_decay_float, default=0.0,
                        help='keep an exponential moving average of the weights with this decay, updated on the device by the '
                             'optimizer step (warm-up min(D, (1 + t) / (10 + t))), validate it beside the live weights and write '
                             'ckps/ema_ckp_<e>.pth / best_ema_ckp.pth; training itself does not depend on it; 0 = off')
    parser.add_argument('--ema_val_interval', type=_positive_int, default=1,
                        help='with --ema_decay: validate the averaged weights every this many epochs (and after the last one)')


WD_HELP = ('weight decay, used as given: with --optimizer adam / momentum an L2 term added to the gradient (the reference\'s 0.0003); '
           'with --optimizer adamw DECOUPLED from the gradient, p *= 1 - lr * wd per step -- not comparable with the L2 value of '
           '--optimizer adam (torch.optim.AdamW defaults to 0.01), and no value has been tuned here: with adamw the default is an '
           'untuned first value')


def add_wd_exempt_flag(parser) -> None:
    """``--wd_exempt_1d`` of both training drivers (resume.py knows the default for state files older than the flag)."""
    parser.add_argument('--wd_exempt_1d', action='store_true', default=False,
                        help='with --optimizer adamw: do not decay parameters with one dimension or none (BatchNorm / GroupNorm '
                             'affine parameters and biases); decided per element inside the update kernel')


def check_optimizer_flags(parser, args) -> None:
    """The check that spans --optimizer and --wd_exempt_1d (an argparse error: exit status 2)."""
    if args.wd_exempt_1d and args.optimizer != 'adamw':
        parser.error(f'--wd_exempt_1d needs --optimizer adamw: the kernels of --optimizer {args.optimizer} decay through the '
                     'gradient and have no exemption')


def log_clip_stats(optimizer, epoch: int, scalars=None, log=None) -> None:
    """Per epoch, where the epoch already synchronised: the gradient-norm statistics of a run with --clip_grad_norm, as a log
    line and as train/grad_norm, train/grad_norm_max, train/grad_clipped_frac; the statistics start over.  Nothing when off."""
    st = optimizer.clip_stats(reset=True)
    if st is None:
        return
    if log is not None:
        log("epoch: {:03d}, grad_norm mean / max: {:.6f} / {:.6f}, {} of {} steps clipped".format(
            epoch, st['mean_norm'], st['max_norm'], st['clipped'], st['steps']))
    if scalars is not None:
        scalars.add('train/grad_norm', st['mean_norm'], epoch)
        scalars.add('train/grad_norm_max', st['max_norm'], epoch)
        scalars.add('train/grad_clipped_frac', st['clipped'] / max(st['steps'], 1), epoch)


class _SlabOptimizer(torch.optim.Optimizer):
    """Shared plumbing: which FlatSlab segments carry gradients this step, and the optimiser state as slab-shaped
    tensors (exposed through state_dict / load_state_dict so a run can be resumed; the reference saves none,
    train_chaos.py:405-413)."""
    STATE_KEYS: tuple = ()

    def _init_state(self):
        self._slabs = {}      # id(FlatSlab) -> dict(<STATE_KEYS tensors>, steps_dev int32[segments], names, flat=FlatSlab)
        self._pending = None  # state handed to load_state_dict before the slab exists
        self._lr_dev = {}     # (index of the param group, device) -> [device scalar, the host value it holds]

    # ---- hyper-parameters the kernels read from the device ------------------------------------------------------
    def lr_scalar(self, group, device) -> torch.Tensor:
        """Device scalar holding ``group['lr']`` (written only when the host value changed: poly_lr_decay sets it per epoch)."""
        # keyed by the group's POSITION: load_state_dict / add_param_group may replace the dict objects, and a
        # captured hipGraph keeps reading the scalar it was captured with -- the scalar of group i must stay the same tensor
        gi = next((i for i, g in enumerate(self.param_groups) if g is group), None)
        if gi is None:
            raise ValueError('lr_scalar: not one of this optimizer\'s param_groups')
        key = (gi, device.index)
        ent = self._lr_dev.get(key)
        lr = float(group['lr'])
        if ent is None:
            ent = [torch.full((1,), lr, device=device, dtype=torch.float32), lr]
            self._lr_dev[key] = ent
        elif ent[1] != lr:
            ent[0].fill_(lr)
            ent[1] = lr
        return ent[0]

    def hyper_ptrs(self) -> tuple:
        """Addresses of the device scalars the step kernels read (part of GraphedStep's capture key: a replay is only valid while
        the captured kernels' scalars are the ones sync_hyper refreshes)."""
        return tuple(sorted((k, v[0].data_ptr()) for k, v in self._lr_dev.items()))

    def sync_hyper(self) -> None:
        """Refresh the device copies of the host-side hyper-parameters (call OUTSIDE a graph capture, before a replay)."""
        for group in self.param_groups:
            for p in group['params']:
                if p.is_cuda:
                    self.lr_scalar(group, p.device)
                    break

    # ---- gradient-norm clipping ---------------------------------------------------------------------------------
    def _clip_buffers(self, flat, state) -> dict:
        """Scratch rows, [norm, coefficient] and the statistics block of one slab: allocated once (their addresses are baked into
        a captured hipGraph), rows for every segment of the slab so that any set of active segments fits."""
        clip = state.get('clip')
        if clip is None:
            dev = flat.params.device
            rows = sum(int(lib.pp_grad_sumsq_rows(b - a)) for a, b in flat.segments.values())
            clip = dict(partial=torch.zeros(rows, device=dev, dtype=torch.float64),
                        out2=torch.zeros(2, device=dev, dtype=torch.float32),
                        stats=torch.zeros(4, device=dev, dtype=torch.float64))      # steps, clipped, sum of norms, max norm
            state['clip'] = clip
        return clip

    def _clip_launch(self, group, flat, state, active, skip, st):
        """With ``group['max_grad_norm']`` set: enqueue the norm of the active segments of `flat` and the clip coefficient;
        returns the address of the coefficient for the ``*_step_clip`` launches (None: clipping is off, nothing was enqueued).
        Segment ranges include the slab's alignment padding: that padding is zero in ``flat.grads`` -- the slab is allocated with
        ``torch.zeros`` and written only through the parameter views, the whole-segment loss-scale removal (0 * x = 0) and the
        all-reduce (a sum of zeros) -- so it adds nothing to the sum of squares (tests/test_gpu_clip.py checks the norm against
        the parameters' own gradients)."""
        max_norm = check_max_grad_norm(group.get('max_grad_norm'))
        if max_norm is None:
            return None
        clip = self._clip_buffers(flat, state)
        rows = 0
        for name, a, b, _ in active:
            lib.pp_grad_sumsq(flat.grads.data_ptr() + 4 * a, b - a, clip['partial'].data_ptr() + 8 * rows, st)
            rows += int(lib.pp_grad_sumsq_rows(b - a))
        lib.pp_grad_clip_finalize(clip['partial'].data_ptr(), rows, max_norm, skip, clip['out2'].data_ptr(),
                                  clip['stats'].data_ptr(), st)
        return clip['out2'].data_ptr() + 4

    def _clip_state(self):
        for state in self._slabs.values():
            if 'clip' in state and any(g.get('max_grad_norm') is not None for g in self.param_groups):
                return state['clip']
        return None

    @property
    def last_grad_norm(self):
        """Global L2 norm of the gradients of the last ``step()``, before clipping: a 1-element fp32 device tensor (no host sync);
        None when ``max_grad_norm`` is off or no step ran yet."""
        clip = self._clip_state()
        return None if clip is None else clip['out2'][0:1]

    @property
    def last_clip_coef(self):
        """The coefficient min(1, max_grad_norm / (norm + 1e-6)) the last ``step()`` applied (device tensor, as last_grad_norm)."""
        clip = self._clip_state()
        return None if clip is None else clip['out2'][1:2]

    def clip_stats(self, reset: bool = False):
        """dict(steps, clipped, mean_norm, max_norm) over the optimizer steps since the last reset (steps the overflow guard
        skipped are not counted); None when ``max_grad_norm`` is off.  Reads the device: call it where the epoch synchronises."""
        clip = self._clip_state()
        if clip is None:
            return None
        steps, clipped, total, mx = clip['stats'].tolist()
        if reset:
            clip['stats'].zero_()
        return dict(steps=int(steps), clipped=int(clipped), mean_norm=total / steps if steps else 0.0, max_norm=mx)

    # ---- EMA of the weights --------------------------------------------------------------------------------------
    def _ema_on(self) -> bool:
        return any(g.get('ema_decay') is not None for g in self.param_groups)

    def _ema_slab(self, state, saved=None) -> torch.Tensor:
        """The shadow slab of one parameter slab: allocated once (its address is baked into a captured hipGraph), bit for bit the
        parameters of that moment -- or `saved`, the shadow of a loaded state."""
        ema = state.get('ema')
        if ema is None:
            ema = state['flat'].params.detach().clone()
            state['ema'] = ema
        if saved is not None:
            ema.copy_(saved.to(ema.device))
        return ema

    def _ema_ptr(self, group, state):
        """Address of the shadow slab for the ``*_step_ema`` launches of `group`; None: ``ema_decay`` is off, today's entry points."""
        if check_ema_decay(group.get('ema_decay')) is None:
            return None
        return self._ema_slab(state).data_ptr()

    @contextlib.contextmanager
    def ema_weights(self):
        """Evaluate on the averaged weights: inside the context the parameter slab holds the EMA and the shadow holds the live
        weights (swapped in place on the device, no third copy); on exit they are swapped back, whatever happened inside.  Only the
        segments the optimizer has updated are swapped -- every other parameter, and every buffer (BatchNorm running statistics),
        stays the live model's.  ``flat.version`` is bumped both ways, so forward-only plans pack the weights they are about to
        use.  Do not train inside the context.  Not re-entrant; not capturable."""
        if not self._ema_on():
            raise RuntimeError('ema_weights(): ema_decay is off')
        if getattr(self, '_ema_swapped', False):
            raise RuntimeError('ema_weights() is not re-entrant: the parameter slab already holds the averaged weights')
        if torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
            raise RuntimeError('ema_weights() cannot run during a stream capture (it reads the step counts on the host)')
        todo = []
        for state in self._slabs.values():
            if 'ema' not in state:
                continue
            flat, done = state['flat'], self._steps_host(state)
            ranges = [flat.segments[name] for name in state['names'] if name in done]
            if ranges:
                todo.append((flat, state['ema'], ranges))

        def swap():
            for flat, ema, ranges in todo:
                with torch.cuda.device(flat.params.device):
                    for a, b in ranges:
                        lib.pp_slab_swap(flat.params.data_ptr() + 4 * a, ema.data_ptr() + 4 * a, b - a, stream_ptr())
                flat.version += 1
        self._ema_swapped = True
        try:
            swap()
            yield self
        finally:
            try:
                swap()
            finally:
                self._ema_swapped = False

    def ema_state_dict(self, model) -> dict:
        """``model.state_dict()`` as it reads inside ``ema_weights()``: the same keys, host tensors (averaged parameters; everything
        the optimizer does not update, the buffers included, from the live model)."""
        with self.ema_weights():
            return {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}

    def _steps_host(self, state) -> dict:
        vals = state['steps_dev'].tolist()                       # one host sync (state_dict / tests only)
        return {name: int(vals[i]) for i, name in enumerate(state['names']) if vals[i] > 0}

    def _set_steps(self, state, steps: dict) -> None:
        vals = [int(steps.get(name, 0)) for name in state['names']]
        state['steps_dev'].copy_(torch.tensor(vals, dtype=torch.int32))

    def _state_for(self, flat) -> dict:
        """The optimiser state of one parameter slab, created on first use: zero moments and step counts -- or what
        load_state_dict left pending -- and, with ``ema_decay``, the shadow slab."""
        state = self._slabs.get(id(flat))
        if state is None:
            state = {k: torch.zeros_like(flat.params) for k in self.STATE_KEYS}
            state['names'] = list(flat.segments)
            state['steps_dev'] = torch.zeros(len(state['names']), device=flat.params.device, dtype=torch.int32)
            state['flat'] = flat
            if self._pending is not None:
                for k in self.STATE_KEYS:
                    state[k].copy_(self._pending[k].to(flat.params.device))
                self._set_steps(state, self._pending['steps'])
            if self._ema_on():
                self._ema_slab(state, None if self._pending is None else self._pending.get('ema'))
            self._pending = None
            self._slabs[id(flat)] = state
        return state

    def ema_shadow(self, flat) -> torch.Tensor:
        """The shadow slab of `flat`, created NOW if no step has run yet (a mean-teacher forward reads it before the first
        update: ConsistencyRegulr.attach_teacher).  Same layout as ``flat.params``; allocated once."""
        if not self._ema_on():
            raise ValueError('ema_shadow(): ema_decay is off (the EMA teacher needs --ema_decay > 0)')
        if not any(p in flat.offsets for g in self.param_groups for p in g['params']):
            raise ValueError('ema_shadow(): this optimizer updates no parameter of that slab')
        if self._slabs and id(flat) not in self._slabs:
            raise RuntimeError('the model was re-flattened after the first optimiser step: the optimiser state belongs to the '
                               'old parameter slab; rebuild the optimiser')
        return self._ema_slab(self._state_for(flat))

    def ema_resync(self, flat) -> None:
        """shadow := parameters on every segment of `flat` the optimizer has not updated yet (step count 0: the average has not
        started there, and ``ema_weights()`` would not swap it in either).  For weights written in place after the shadow was
        created -- ``load_state_dict``, ``--init_from`` -- so that a reader of the shadow sees them.  Reads the step counts on
        the host: not for the training loop."""
        state = self._slabs.get(id(flat))
        if state is None or 'ema' not in state or getattr(self, '_ema_swapped', False):
            return
        done = self._steps_host(state)
        with torch.no_grad():
            for name in state['names']:
                if name not in done:
                    a, b = flat.segments[name]
                    state['ema'][a:b].copy_(flat.params[a:b])

    def _segments_with_grads(self, group):
        todo = {}
        for p in group['params']:
            if p.grad is None:
                continue                      # torch.optim skips parameters without a gradient
            flat = getattr(p, '_pp_flat', None)
            if flat is None or not flat.owns(p) or p.grad.data_ptr() != flat.grad_views[p].data_ptr():
                raise RuntimeError(f'{type(self).__name__} only updates parameters that live in a pacingpseudo_amd FlatSlab '
                                   '(build the model with pacingpseudo_amd and call .cuda() before training)')
            todo.setdefault(id(flat), (flat, set()))[1].add(p)
        for flat, have in todo.values():
            if self._slabs and id(flat) not in self._slabs:
                raise RuntimeError('the model was re-flattened (.cuda()/.to() after the first optimiser step): the '
                                   'optimiser state belongs to the old parameter slab; rebuild the optimiser or carry '
                                   'the state over with state_dict() / load_state_dict()')
            state = self._state_for(flat)
            active = []
            for i, (name, (a, b)) in enumerate(flat.segments.items()):
                ps = flat.seg_params[name]
                n_have = sum(1 for p in ps if p in have)
                if n_have == 0:
                    continue
                if n_have != len(ps):
                    raise RuntimeError(f'segment {name}: only {n_have}/{len(ps)} parameters carry a gradient')
                active.append((name, a, b, state['steps_dev'].data_ptr() + 4 * i))
            yield flat, state, active

    def state_dict(self):
        sd = dict(param_groups=[{k: v for k, v in g.items() if k != 'params'} for g in self.param_groups])
        sd['slabs'] = [dict({k: st[k].detach().cpu() for k in self.STATE_KEYS}, steps=self._steps_host(st))
                       for st in self._slabs.values()]
        if self._ema_on():                    # off: exactly the keys above
            for out, st in zip(sd['slabs'], self._slabs.values()):
                if 'ema' in st:
                    out['ema'] = st['ema'].detach().cpu()
        return sd

    def load_state_dict(self, sd):
        for g, saved in zip(self.param_groups, sd['param_groups']):
            g.update(saved)
            g['max_grad_norm'] = check_max_grad_norm(saved.get('max_grad_norm'))      # a state dict older than the key: off
            g['ema_decay'] = check_ema_decay(saved.get('ema_decay'))                  # the same
        if sd.get('slabs'):
            if len(sd['slabs']) != 1:
                raise ValueError('expected the state of exactly one parameter slab')
            st = sd['slabs'][0]
            if self._slabs:
                cur = next(iter(self._slabs.values()))
                for k in self.STATE_KEYS:
                    cur[k].copy_(st[k].to(cur[k].device))
                self._set_steps(cur, st['steps'])
                if self._ema_on():            # a state without a shadow: the average starts from the current parameters
                    self._ema_slab(cur, st['ema'] if 'ema' in st else cur['flat'].params)
            else:
                self._pending = st


class FusedAdam(_SlabOptimizer):
    STATE_KEYS = ('m', 'v')

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, max_grad_norm=None, ema_decay=None):
        if lr < 0 or eps < 0 or weight_decay < 0:
            raise ValueError('invalid Adam hyper-parameter')
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay,
                                      max_grad_norm=check_max_grad_norm(max_grad_norm), ema_decay=check_ema_decay(ema_decay)))
        self._init_state()

    @torch.no_grad()
    def step(self, closure=None):
        if closure is not None:
            raise NotImplementedError('closures are not supported')
        st = stream_ptr()
        with prof_range('optimizer: Adam'):
            for group in self.param_groups:
                b1, b2 = group['betas']
                for flat, state, active in self._segments_with_grads(group):
                    skip = flat.guard.data_ptr() if getattr(flat, 'guard_on', False) else None      # 16-bit storage: overflow guard
                    lr_dev = self.lr_scalar(group, flat.params.device).data_ptr()
                    clip_dev = self._clip_launch(group, flat, state, active, skip, st)
                    ema = self._ema_ptr(group, state)
                    for j, (name, a, b, step_ptr) in enumerate(active):
                        common = (flat.params.data_ptr() + 4 * a, flat.grads.data_ptr() + 4 * a,
                                  state['m'].data_ptr() + 4 * a, state['v'].data_ptr() + 4 * a, b - a,
                                  float(group['lr']), lr_dev, float(b1), float(b2), float(group['eps']),
                                  float(group['weight_decay']), step_ptr, skip, 1 if j == 0 else 0)
                        if ema is not None:
                            lib.pp_adam_step_ema(*common, ema + 4 * a, group['ema_decay'], clip_dev, st)
                        elif clip_dev is None:
                            lib.pp_adam_step_dev(*common, st)
                        else:
                            lib.pp_adam_step_clip(*common, clip_dev, st)
                    flat.version += 1
        return None


def check_adamw_hyper(lr, betas, eps, weight_decay) -> None:
    """What libpacingpseudo_opt.so would refuse at the first step, refused when the optimizer is built."""
    for name, value in (('lr', lr), ('eps', eps), ('weight_decay', weight_decay)):
        value = float(value)
        if not (value >= 0.0 and value < math.inf):          # NaN compares false
            raise ValueError(f'invalid AdamW hyper-parameter: {name} must be finite and >= 0, got {value!r}')
    if len(betas) != 2 or not all(0.0 <= float(b) < 1.0 for b in betas):
        raise ValueError(f'invalid AdamW hyper-parameter: betas must be two values in [0, 1), got {betas!r}')


def decay_exempt_mask(flat) -> torch.Tensor:
    """One byte per element of ``flat.params`` (uint8, on the host): 1 for every element of a parameter with ``ndim <= 1`` -- the
    affine parameters of BatchNorm / GroupNorm and the biases, which ``FusedAdamW(exempt_1d=True)`` does not decay -- 0 for every
    other parameter and for the alignment padding (it holds zeros, and zeros stay zeros under both the decay and the Adam move).
    A marked run starts wherever its tensor starts: FlatSlab aligns segments, not parameters."""
    mask = torch.zeros(int(flat.numel), dtype=torch.uint8)
    for p, off in flat.offsets.items():
        if p.ndim <= 1:
            mask[off:off + p.numel()] = 1
    return mask


class FusedAdamW(_SlabOptimizer):
    """``torch.optim.AdamW(params, lr, betas, eps, weight_decay)`` (non-amsgrad): the decay is decoupled from the gradient,
    ``p *= 1 - lr * weight_decay`` before the Adam move, and never enters the moments.  ``exempt_1d``: parameters with
    ``ndim <= 1`` are not decayed; the decision is taken per ELEMENT inside the kernel from a byte mask laid over the slab
    (``decay_exempt_mask``), because those tensors are interleaved with the convolution weights inside the segments the kernel
    is launched over.  Everything else -- device-side step counts and learning rate, the overflow guard, ``max_grad_norm``,
    ``ema_decay``, ``state_dict()`` -- is ``FusedAdam``'s.  The update kernels are libpacingpseudo_opt.so's (``_opt.py``); the
    norm kernels of the clipping stay in the per-step library."""
    STATE_KEYS = ('m', 'v')

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, exempt_1d=False, max_grad_norm=None,
                 ema_decay=None):
        check_adamw_hyper(lr, betas, eps, weight_decay)
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, exempt_1d=bool(exempt_1d),
                                      max_grad_norm=check_max_grad_norm(max_grad_norm), ema_decay=check_ema_decay(ema_decay)))
        self._init_state()

    def load_state_dict(self, sd):
        super().load_state_dict(sd)
        for g, saved in zip(self.param_groups, sd['param_groups']):
            g['exempt_1d'] = bool(saved.get('exempt_1d', False))          # a state dict older than the key: off

    def _exempt_ptr(self, group, flat, state):
        """Address of the slab's exemption mask on the device, or None with ``exempt_1d`` off (the kernel then reads no mask).
        Built once, on first use, next to m and v, and never reallocated: its address is baked into a captured hipGraph."""
        if not group.get('exempt_1d', False):
            return None
        mask = state.get('exempt')
        if mask is None:
            mask = decay_exempt_mask(flat).to(flat.params.device)
            state['exempt'] = mask
        return mask.data_ptr()

    @torch.no_grad()
    def step(self, closure=None):
        if closure is not None:
            raise NotImplementedError('closures are not supported')
        from ._opt import opt
        st = stream_ptr()
        with prof_range('optimizer: AdamW'):
            for group in self.param_groups:
                b1, b2 = group['betas']
                for flat, state, active in self._segments_with_grads(group):
                    skip = flat.guard.data_ptr() if getattr(flat, 'guard_on', False) else None      # 16-bit storage: overflow guard
                    lr_dev = self.lr_scalar(group, flat.params.device).data_ptr()
                    exempt = self._exempt_ptr(group, flat, state)
                    clip_dev = self._clip_launch(group, flat, state, active, skip, st)
                    ema = self._ema_ptr(group, state)
                    for j, (name, a, b, step_ptr) in enumerate(active):
                        common = (flat.params.data_ptr() + 4 * a, flat.grads.data_ptr() + 4 * a,
                                  state['m'].data_ptr() + 4 * a, state['v'].data_ptr() + 4 * a, b - a,
                                  float(group['lr']), lr_dev, float(b1), float(b2), float(group['eps']),
                                  float(group['weight_decay']), step_ptr, skip, 1 if j == 0 else 0,
                                  None if exempt is None else exempt + a)
                        if ema is not None:
                            opt.popt_adamw_step_ema(*common, ema + 4 * a, group['ema_decay'], clip_dev, st)
                        elif clip_dev is None:
                            opt.popt_adamw_step(*common, st)
                        else:
                            opt.popt_adamw_step_clip(*common, clip_dev, st)
                    flat.version += 1
        return None


class FusedSGD(_SlabOptimizer):
    """``torch.optim.SGD(params, lr, momentum, weight_decay)`` (train_chaos.py:220-221, ``--optimizer momentum``):
    L2-coupled decay, dampening 0, no Nesterov, momentum buffer initialised with the first gradient."""
    STATE_KEYS = ('momentum_buffer',)

    def __init__(self, params, lr=1e-3, momentum=0.0, weight_decay=0.0, max_grad_norm=None, ema_decay=None):
        if lr < 0 or momentum < 0 or weight_decay < 0:
            raise ValueError('invalid SGD hyper-parameter')
        super().__init__(params, dict(lr=lr, momentum=momentum, weight_decay=weight_decay,
                                      max_grad_norm=check_max_grad_norm(max_grad_norm), ema_decay=check_ema_decay(ema_decay)))
        self._init_state()

    @torch.no_grad()
    def step(self, closure=None):
        if closure is not None:
            raise NotImplementedError('closures are not supported')
        st = stream_ptr()
        for group in self.param_groups:
            for flat, state, active in self._segments_with_grads(group):
                skip = flat.guard.data_ptr() if getattr(flat, 'guard_on', False) else None
                lr_dev = self.lr_scalar(group, flat.params.device).data_ptr()
                clip_dev = self._clip_launch(group, flat, state, active, skip, st)
                ema = self._ema_ptr(group, state)
                for j, (name, a, b, step_ptr) in enumerate(active):
                    common = (flat.params.data_ptr() + 4 * a, flat.grads.data_ptr() + 4 * a,
                              state['momentum_buffer'].data_ptr() + 4 * a, b - a, float(group['lr']), lr_dev,
                              float(group['momentum']), float(group['weight_decay']), step_ptr, skip, 1 if j == 0 else 0)
                    if ema is not None:
                        lib.pp_sgd_momentum_step_ema(*common, ema + 4 * a, group['ema_decay'], clip_dev, st)
                    elif clip_dev is None:
                        lib.pp_sgd_momentum_step_dev(*common, st)
                    else:
                        lib.pp_sgd_momentum_step_clip(*common, clip_dev, st)
                flat.version += 1
        return None
