"""Epoch-boundary run state for the training drivers (``--state_interval N`` / ``--resume PATH``).

``ckps/ckp_<epoch>.pth`` and ``best_ckp.pth`` keep the reference's layout (``model.state_dict()`` only; inference.py and the
reference load them).  A state file ``ckps/state_<epoch>.pth`` holds everything else a run keeps in its process, so that a
run stopped after epoch e and resumed ends exactly where the uninterrupted run ends, bit for bit: the model (BatchNorm buffers
and memory bank included), the optimiser (slab moments, per-segment step counts), the 16-bit storage loss scale and its
overflow-guard counters, eval mode, the best-Dice bookkeeping, ``valdice[:e+1]`` and, for every rank, the python / numpy /
torch CPU / torch CUDA generators and the ``DeviceAugmenter``'s host ``RandomState``.

Everything in the file is a tensor or a plain python value, so it loads with ``torch.load(weights_only=True)``.
"""
from __future__ import annotations

import glob
import json
import os
import random
import re
import tempfile

import numpy as np
import torch

FORMAT = 'pacingpseudo_amd run state'
VERSION = 1

# flags that select where a run writes or how its host side is organised, never what it computes: they may differ on resume.
# (--graph_step replays the eager step bit for bit; --root / --tag only name the run directory, and a resumed run continues in
# the directory its state file belongs to; --gpu_augment is an accepted no-op; --ema_val_interval only says how often the
# averaged weights are looked at.)
# (--init_from / --init_reset_head only say where a FRESH run takes its first weights from; a resumed run takes them from the
# state file.  --freeze_encoder changes what is trained and is compared.)
MAY_DIFFER = frozenset({'gpu', 'num_workers', 'graph_step', 'resume', 'state_interval', 'root', 'tag', 'gpu_augment',
                        'ema_val_interval', 'init_from', 'init_reset_head'})
# flags that are younger than the state-file format, with their parser defaults: a state file written before the flag existed
# lacks the key, and the run it describes computed what the default computes
ABSENT_DEFAULTS = {'clip_grad_norm': 0.0, 'ema_decay': 0.0, 'ema_val_interval': 1, 'cr_teacher': 'none',
                   'do_loss_crf': False, 'loss_crf_weight': 0.1, 'ramp_up_loss_crf': False, 'crf_radius': 5, 'crf_dilation': 1,
                   'crf_sigma_xy': 6.0, 'crf_sigma_rgb': 0.1,
                   'do_loss_nc': False, 'loss_nc_weight': 0.1, 'ramp_up_loss_nc': False, 'nc_radius': 5, 'nc_dilation': 1,
                   'nc_sigma_xy': 6.0, 'nc_sigma_rgb': 0.1,
                   'do_loss_ms': False, 'loss_ms_weight': 0.1, 'ramp_up_loss_ms': False, 'ms_tv_weight': 1.0,
                   'freeze_encoder': 0, 'init_from': None, 'init_reset_head': False,
                   'rw_scribbles': False, 'rw_beta': 13.0, 'rw_threshold': 0.9, 'rw_eps': 1e-4, 'rw_tol': 1e-6, 'rw_max_iters': 10000,
                   'rw_refresh': 0, 'rw_refresh_start': 0, 'rw_prior_gamma': 0.1,
                   'cr_uncertainty': 0, 'cr_uncertainty_sigma': 0.1, 'cr_uncertainty_clip': 0.2, 'cr_uncertainty_start': 0.75,
                   'do_loss_boundary': False, 'loss_boundary_weight': 0.01, 'ramp_up_loss_boundary': 0,
                   'geo_scribbles': False, 'geo_lambda': 20.0, 'geo_ratio': 0.25, 'geo_max_dist': float('inf'), 'geo_max_sweeps': 100000,
                   'wd_exempt_1d': False,
                   'do_loss_lovasz': False, 'loss_lovasz_weight': 1.0, 'ramp_up_loss_lovasz': 0, 'lovasz_per_image': False}
# attributes the drivers add to the namespace after parsing (not flags)
_DERIVED = frozenset({'child', 'train_ls', 'val_ls'})


class ResumeError(ValueError):
    """A state file that cannot be resumed from, or a command line that does not match it."""


def add_flags(parser) -> None:
    parser.add_argument('--state_interval', type=int, default=0,
                        help='write ckps/state_<epoch>.pth (everything needed to resume the run bit for bit) every this many '
                             'epochs and after the last one; 0 = never')
    parser.add_argument('--resume', type=str, default=None,
                        help='continue the run of this state file (or of the highest-numbered ckps/state_*.pth of this run '
                             'directory) in its own directory, from the epoch after the saved one')


def flag_dict(args) -> dict:
    """The parsed (and preset-resolved) flags of a run, without the attributes the drivers derive from them."""
    return {k: v for k, v in vars(args).items() if k not in _DERIVED}


# ---- files ---------------------------------------------------------------------------------------------------------------
def state_path(run_dir: str, epoch: int) -> str:
    return os.path.join(run_dir, 'ckps', f'state_{epoch:d}.pth')


def resolve(path: str) -> str:
    """A state file as given, or the highest-numbered ``ckps/state_<e>.pth`` of a run directory."""
    if os.path.isdir(path):
        found = []
        for f in glob.glob(os.path.join(path, 'ckps', 'state_*.pth')):
            m = re.fullmatch(r'state_(\d+)\.pth', os.path.basename(f))
            if m:
                found.append((int(m.group(1)), f))
        if not found:
            raise ResumeError(f'--resume {path}: the run directory holds no ckps/state_<epoch>.pth '
                              '(state files are written with --state_interval N)')
        return max(found)[1]
    if not os.path.isfile(path):
        raise ResumeError(f'--resume {path}: no such state file or run directory')
    return path


def run_dir_of(path: str) -> str:
    """The run directory a state file belongs to (<run>/ckps/state_<e>.pth)."""
    return os.path.dirname(os.path.dirname(os.path.abspath(path)))


def atomic_save(obj, path: str) -> None:
    """torch.save through a temporary file in the same directory + os.replace: a kill during the write never leaves a
    truncated file under `path`."""
    d = os.path.dirname(os.path.abspath(path))
    fd, tmp = tempfile.mkstemp(prefix='.' + os.path.basename(path) + '.', suffix='.tmp', dir=d)
    try:
        with os.fdopen(fd, 'wb') as f:
            torch.save(obj, f)
            f.flush()
            os.fsync(f.fileno())
        os.replace(tmp, path)
    except BaseException:
        if os.path.exists(tmp):
            os.unlink(tmp)
        raise


def load(path: str) -> dict:
    """Read and validate a state file (CPU tensors)."""
    try:
        st = torch.load(path, map_location='cpu', weights_only=True)
    except Exception as e:                      # truncated / not a torch file / foreign pickle
        raise ResumeError(f'--resume {path}: not a readable run-state file ({type(e).__name__}: {str(e).splitlines()[0] if str(e) else ""})') from None
    if not isinstance(st, dict) or st.get('format') != FORMAT:
        raise ResumeError(f'--resume {path}: not a run-state file (ckps/state_<epoch>.pth written with --state_interval); '
                          'ckp_*.pth / best_ckp.pth hold model weights only and cannot be resumed from')
    if st.get('version') != VERSION:
        raise ResumeError(f'--resume {path}: unknown state format version {st.get("version")!r} (this build reads version {VERSION})')
    return st


def check_compatible(saved: dict, new: dict, world: int, saved_world: int) -> None:
    """Refuse a resume whose command line would compute something else than the saved run: every flag outside MAY_DIFFER
    must match, and so must the number of ranks."""
    if int(world) != int(saved_world):
        raise ResumeError(f'--resume: the run was saved with world size {saved_world} and is resumed with world size {world}; '
                          'the data shards, batch statistics and RNG streams are per rank, so the world size must match')
    keys = sorted((set(saved) | set(new)) - MAY_DIFFER)
    saved = {**{k: v for k, v in ABSENT_DEFAULTS.items() if k in new}, **saved}
    diff = [k for k in keys if saved.get(k) != new.get(k)]
    if diff:
        raise ResumeError('--resume: these flags differ from the saved run and would change what it computes: '
                          + ', '.join(f'--{k} (saved {saved.get(k)!r}, now {new.get(k)!r})' for k in diff))


def truncate_scalars(path: str, last_epoch: int) -> None:
    """Keep the lines of tb_summary/scalars.jsonl whose step is <= last_epoch (an epoch cut short leaves none behind)."""
    if not os.path.isfile(path):
        return
    keep = []
    with open(path) as f:
        for line in f:
            try:
                rec = json.loads(line)
            except ValueError:
                continue                        # a line the killed run did not finish
            if int(rec.get('step', last_epoch + 1)) <= last_epoch:
                keep.append(line if line.endswith('\n') else line + '\n')
    d = os.path.dirname(os.path.abspath(path))
    fd, tmp = tempfile.mkstemp(prefix='.scalars.', suffix='.tmp', dir=d)
    with os.fdopen(fd, 'w') as f:
        f.writelines(keep)
    os.replace(tmp, path)


# ---- --rw_refresh: the pseudo-label maps in force ---------------------------------------------------------------------------
# The state file's format does not change: a refresh at epoch t leaves <run dir>/rw_refresh/maps_<t>.npz behind, and a run resumed
# from state_<e> trains on the maps of the largest refresh epoch t <= e (a refresh due at e + 1 is recomputed from the restored
# weights like any other work of that epoch).
def refresh_maps_path(run_dir: str, epoch: int) -> str:
    return os.path.join(run_dir, 'rw_refresh', f'maps_{epoch:d}.npz')


def save_refresh_maps(path: str, maps, report: dict, params: dict) -> None:
    """Compressed uint8 maps (one flat array + the (h, w) of every slice) with the refresh's report and parameters, through a
    temporary file in the same directory + os.replace."""
    d = os.path.dirname(os.path.abspath(path))
    os.makedirs(d, exist_ok=True)
    flat = np.concatenate([np.asarray(m, dtype=np.uint8).ravel() for m in maps]) if len(maps) else np.zeros(0, np.uint8)
    shapes = np.asarray([m.shape for m in maps], dtype=np.int32).reshape(len(maps), 2)
    fd, tmp = tempfile.mkstemp(prefix='.' + os.path.basename(path) + '.', suffix='.tmp', dir=d)
    try:
        with os.fdopen(fd, 'wb') as f:
            np.savez_compressed(f, maps=flat, shapes=shapes, **{'report_' + k: v for k, v in report.items()},
                                **{'param_' + k: v for k, v in params.items()})
            f.flush()
            os.fsync(f.fileno())
        os.replace(tmp, path)
    except BaseException:
        if os.path.exists(tmp):
            os.unlink(tmp)
        raise


def read_refresh_maps(path: str) -> list:
    """The per-slice uint8 (h, w) maps of a file written by save_refresh_maps."""
    with np.load(path) as z:
        flat, shapes = z['maps'], z['shapes']
    off = np.concatenate([[0], np.cumsum(shapes[:, 0].astype(np.int64) * shapes[:, 1])])
    return [flat[off[i]:off[i + 1]].reshape(int(shapes[i, 0]), int(shapes[i, 1])) for i in range(len(shapes))]


def load_refresh_maps(run_dir: str, epoch: int, every: int, start: int, shapes):
    """The maps a run resumed from state_<epoch> trains on, or None when no refresh happened up to that epoch."""
    if not every or epoch < start:
        return None
    t = start + (epoch - start) // every * every
    path = refresh_maps_path(run_dir, t)
    if not os.path.isfile(path):
        raise ResumeError(f'--resume: {path} is missing: the pseudo-labels in force after epoch {epoch} were written there by the '
                          f'refresh at epoch {t} (--rw_refresh {every}), and the run cannot be continued without them')
    maps = read_refresh_maps(path)
    if [tuple(m.shape) for m in maps] != [tuple(s) for s in shapes]:
        raise ResumeError(f'--resume: {path} does not hold one map per training slice of this data set')
    return maps


# ---- random generators -----------------------------------------------------------------------------------------------------
def _np_state_out(s):
    return (s[0], torch.from_numpy(s[1].astype(np.int64)), int(s[2]), int(s[3]), float(s[4]))


def _np_state_in(s):
    return (s[0], s[1].numpy().astype(np.uint32), int(s[2]), int(s[3]), float(s[4]))


def rng_states(device, augmenter=None) -> dict:
    return dict(python=random.getstate(), numpy=_np_state_out(np.random.get_state()), torch=torch.get_rng_state(),
                cuda=torch.cuda.get_rng_state(device),
                augmenter=_np_state_out(augmenter.rng.get_state()) if augmenter is not None else None)


def set_rng_states(st: dict, device, augmenter=None) -> None:
    random.setstate(st['python'])
    np.random.set_state(_np_state_in(st['numpy']))
    torch.set_rng_state(st['torch'])
    torch.cuda.set_rng_state(st['cuda'], device)
    if augmenter is not None:
        augmenter.rng.set_state(_np_state_in(st['augmenter']))


def gather_rng_states(device, augmenter, world: int) -> list:
    """Every rank's generator states, in rank order (a collective when world > 1: every rank calls it)."""
    mine = rng_states(device, augmenter)
    if world == 1:
        return [mine]
    import torch.distributed as dist
    out = [None] * world
    dist.all_gather_object(out, mine)
    return out


def prime_persistent_loaders(loaders) -> None:
    """A loader with persistent workers draws its worker base seed from the torch default generator once, when its iterator
    is created (epoch 0 of an uninterrupted run); every epoch draws the sampler's seed.  A resumed process creates the
    iterators here, BEFORE the saved generator state is restored, so that the restored state is next drawn from by the first
    resumed epoch's shuffle, as in the uninterrupted run.  The prefetched batches of this iterator are dropped by the
    iterator's reset at the start of that epoch."""
    for loader in loaders:
        if loader.num_workers > 0 and loader.persistent_workers:
            iter(loader)


# ---- the state file ----------------------------------------------------------------------------------------------------------
def capture(args, epoch: int, model, optimizer, best, valdice, rngs, world: int, ema=None) -> dict:
    """`ema` (runs with --ema_decay only): (dict(avg, epoch, avg_class) of the best averaged-weights validation, valdice_ema);
    the shadow slab itself travels in ``optimizer.state_dict()``.  Without it the state has exactly the keys it always had."""
    flat = getattr(model, 'flat', None)
    engine = getattr(model, 'engine', None)
    best_avg, best_epoch, best_avg_class = best
    extra = {}
    if ema is not None:
        best_ema, valdice_ema = ema
        extra = dict(best_ema_avg=float(best_ema['avg']), best_ema_epoch=int(best_ema['epoch']),
                     best_ema_avg_class=[float(v) for v in best_ema['avg_class']],
                     valdice_ema=torch.from_numpy(np.asarray(valdice_ema[:epoch + 1], dtype=np.float64).copy()))
    if engine is not None and getattr(engine, 'unc', None) is not None:
        # --cr_uncertainty only: (seed, step) of the noise generator as rank 0 holds them (the other ranks differ in the seed, which
        # they re-derive from --seed and their rank; the step is the same everywhere)
        extra['uncertainty_state'] = [int(v) for v in engine.uncertainty_state()]
    return dict(
        **extra,
        format=FORMAT, version=VERSION, args=flag_dict(args), world_size=int(world), epoch=int(epoch),
        model={k: v.detach().cpu() for k, v in model.state_dict().items()},
        optimizer=optimizer.state_dict(),
        loss_scale=float(engine.loss_scale) if engine is not None else None,
        guard=flat.guard.detach().cpu() if flat is not None else None,
        skipped_logged=int(getattr(flat, '_skipped_logged', 0)) if flat is not None else 0,
        training=bool(model.training),
        best_avg=float(best_avg), best_epoch=int(best_epoch), best_avg_class=[float(v) for v in best_avg_class],
        valdice=torch.from_numpy(np.asarray(valdice[:epoch + 1], dtype=np.float64).copy()),
        rng=rngs)


def restore(st: dict, model, optimizer, valdice):
    """Load the model / optimiser / loss-scale state of `st` into a freshly built run (in place: the flat parameter slab and
    every pointer the engine baked stay valid).  Returns (best_avg, best_epoch, best_avg_class)."""
    model.load_state_dict(st['model'])
    if not st['training']:
        model.eval()
    optimizer.load_state_dict(st['optimizer'])
    engine = getattr(model, 'engine', None)
    if engine is not None and st.get('loss_scale') is not None:
        engine.set_loss_scale(st['loss_scale'])
    if engine is not None and getattr(engine, 'unc', None) is not None and st.get('uncertainty_state') is not None:
        # the saved STEP into the engine's state buffer, in place, before the first step; the seed is this rank's own
        engine.set_uncertainty_state(engine.uncertainty_state()[0], int(st['uncertainty_state'][1]))
    flat = getattr(model, 'flat', None)
    if flat is not None and st.get('guard') is not None:
        flat.guard.copy_(st['guard'].to(flat.guard.device))
        flat._skipped_logged = int(st['skipped_logged'])
    e = int(st['epoch'])
    valdice[:e + 1] = st['valdice'].numpy()
    return st['best_avg'], st['best_epoch'], list(st['best_avg_class'])


def restore_ema(st: dict, valdice_ema) -> dict:
    """The best-EMA bookkeeping of a run with --ema_decay (restore() has loaded the shadow slab with the optimizer)."""
    e = int(st['epoch'])
    valdice_ema[:e + 1] = st['valdice_ema'].numpy()
    return dict(avg=st['best_ema_avg'], epoch=st['best_ema_epoch'], avg_class=list(st['best_ema_avg_class']))


def open_state(parser, args, world: int):
    """--resume: (state file, its contents), checked against this command line before anything touches the GPU.  A refusal
    is a usage error of `parser` (message on stderr, exit status 2)."""
    try:
        path = resolve(args.resume)
        st = load(path)
        check_compatible(st['args'], flag_dict(args), world, st['world_size'])
    except ResumeError as e:
        parser.error(str(e))
    return path, st
