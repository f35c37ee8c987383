"""--resume on the MI355X: a run stopped after epoch e and resumed from ckps/state_<e>.pth ends bit for bit where the
uninterrupted run ends -- the final checkpoint, best_ckp.pth, valdice.npz, every scalar and the final state file's model,
optimiser and generator states.

Each case runs the uninterrupted run with --state_interval 1, copies its run directory, deletes from the copy what was written
after epoch e, and resumes the copy in a fresh process (the drivers run as subprocesses, each under its own timeout).
Synthetic data and the small shape of test_gpu_graph.py with the full flags."""
import glob
import json
import os
import shutil
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ['--synthetic', '16', '--batch_size', '4', '--image_size', '64']
FULL = ['--session', 'Experiment', '--do_loss_ent', '--do_decoder_consistency', '--do_aux_path', '--do_memory']
RUN_TIMEOUT = 300                     # one 3-epoch driver run of this size takes well under a minute


def _driver(script, argv, env=None, nproc=None):
    env = dict(os.environ, **(env or {}))
    if nproc:
        s = socket.socket()
        s.bind(('127.0.0.1', 0))
        port = s.getsockname()[1]
        s.close()
        cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', str(nproc),
               '--master-addr', '127.0.0.1', '--master-port', str(port), os.path.join(ROOT, script)] + argv
    else:
        for k in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'LOCAL_WORLD_SIZE'):
            env.pop(k, None)
        cmd = [sys.executable, os.path.join(ROOT, script)] + argv
    return subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=RUN_TIMEOUT * (nproc or 1))


def _run(script, argv, root, tag, session='Experiment', **kw):
    r = _driver(script, argv + ['--tag', tag, '--root', str(root)], **kw)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-5000:]
    runs = glob.glob(os.path.join(str(root), 't1', session, f'{session}-*-fold1-{tag}'))
    assert len(runs) == 1, runs
    return runs[0]


def _load(path):
    return torch.load(path, map_location='cpu', weights_only=True)


def _trimmed_copy(run, src_root, dst_root, e, last):
    """The run directory as a run killed after epoch e's state file left it."""
    dst = os.path.join(str(dst_root), os.path.relpath(run, str(src_root)))
    shutil.copytree(run, dst)
    for k in range(e + 1, last + 1):
        for name in (f'state_{k}.pth', f'ckp_{k}.pth'):
            p = os.path.join(dst, 'ckps', name)
            if os.path.exists(p):
                os.remove(p)
    os.remove(os.path.join(dst, 'valdice.npz'))
    log = open(os.path.join(dst, 'log.txt')).read().splitlines(keepends=True)
    cut = next(i for i, line in enumerate(log) if f'val: {e:03d},' in line) + 2          # + the per-class Dice line
    with open(os.path.join(dst, 'log.txt'), 'w') as f:
        f.writelines(log[:cut])
    if _load(os.path.join(run, 'ckps', f'state_{last}.pth'))['best_epoch'] > e:
        os.remove(os.path.join(dst, 'best_ckp.pth'))         # written after epoch e: the resumed run must write it again
    return dst


def _scalars(run):
    out = {}
    for line in open(os.path.join(run, 'tb_summary', 'scalars.jsonl')):
        r = json.loads(line)
        key = (r['tag'], r['step'])
        assert key not in out, f'{key} logged twice in {run}'
        out[key] = r['value']
    return out


def _assert_equal_tree(a, b, where):
    if torch.is_tensor(a):
        assert torch.is_tensor(b) and a.dtype == b.dtype and torch.equal(a, b), where
    elif isinstance(a, dict):
        assert set(a) == set(b), (where, set(a) ^ set(b))
        for k in a:
            _assert_equal_tree(a[k], b[k], f'{where}.{k}')
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), where
        for i, (x, y) in enumerate(zip(a, b)):
            _assert_equal_tree(x, y, f'{where}[{i}]')
    else:
        assert a == b, (where, a, b)


def _assert_same_run(full, resumed, last):
    for name in (f'ckps/ckp_{last}.pth', 'best_ckp.pth'):
        sa, sb = _load(os.path.join(full, name)), _load(os.path.join(resumed, name))
        assert list(sa) == list(sb), name
        for k in sa:
            assert torch.equal(sa[k], sb[k]), (name, k)
    va, vb = np.load(os.path.join(full, 'valdice.npz'))['valdice'], np.load(os.path.join(resumed, 'valdice.npz'))['valdice']
    assert va.shape == (last + 1,) and np.array_equal(va, vb), (va, vb)
    assert _scalars(full) == _scalars(resumed)
    fa, fb = _load(os.path.join(full, 'ckps', f'state_{last}.pth')), _load(os.path.join(resumed, 'ckps', f'state_{last}.pth'))
    for key in ('model', 'optimizer', 'loss_scale', 'guard', 'skipped_logged', 'training', 'best_avg', 'best_epoch',
                'best_avg_class', 'valdice', 'rng', 'epoch', 'world_size'):
        _assert_equal_tree(fa[key], fb[key], key)
    return fa


def _resume_case(tmp_path, script, argv, e, last, resume_extra=(), session='Experiment', **kw):
    full = _run(script, argv + ['--state_interval', '1'], tmp_path / 'full', 'r', session=session, **kw)
    copy = _trimmed_copy(full, tmp_path / 'full', tmp_path / 'resumed', e, last)
    r = _driver(script, argv + list(resume_extra) + ['--state_interval', '1', '--tag', 'r', '--root', str(tmp_path / 'resumed'),
                                                     '--resume', os.path.join(copy, 'ckps', f'state_{e}.pth')], **kw)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-5000:]
    assert sorted(os.listdir(os.path.dirname(copy))) == [os.path.basename(copy)]      # no new run directory
    return full, copy, _assert_same_run(full, copy, last)


@pytest.fixture(scope='module')
def gpu_augment_run(tmp_path_factory):
    """Case 1's uninterrupted run: the default GPU-augmentation path with persistent loader workers and Dropout2d masks."""
    tmp = tmp_path_factory.mktemp('resume_gpu_aug')
    argv = SMALL + FULL + ['--epoch', '3', '--num_workers', '2', '--aux_drop_prob', '0.5']
    return tmp, argv, _run('train_chaos.py', argv + ['--state_interval', '1'], tmp / 'full', 'r')


def test_resume_across_the_batchnorm_switch_with_persistent_workers(gpu_augment_run):
    """Resumed from state_0: the train->eval BatchNorm switch, the loader's shuffle draws (persistent workers draw their base seed
    at epoch 0 only) and the CUDA generator of the Dropout2d masks."""
    tmp, argv, full = gpu_augment_run
    copy = _trimmed_copy(full, tmp / 'full', tmp / 'resumed', 0, 2)
    r = _driver('train_chaos.py', argv + ['--state_interval', '1', '--tag', 'r', '--root', str(tmp / 'resumed'), '--resume', copy])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-5000:]
    # the directory form picked state_0 (the only one left); the log goes on at epoch 1
    st = _assert_same_run(full, copy, 2)
    assert st['training'] is False
    log = open(os.path.join(copy, 'log.txt')).read()
    head, tail = log.split('resumed from', 1)
    assert 'epoch: 000' in head and 'epoch: 001' not in head
    assert 'epoch: 001' in tail and 'epoch: 002' in tail and 'epoch: 000' not in tail


def test_writing_state_files_does_not_change_the_run(gpu_augment_run):
    """--state_interval 1 against the same run without it: saving must not draw from any generator."""
    tmp, argv, full = gpu_augment_run
    plain = _run('train_chaos.py', argv, tmp / 'plain', 'r')
    assert not glob.glob(os.path.join(plain, 'ckps', 'state_*.pth'))
    sa, sb = _load(os.path.join(full, 'ckps', 'ckp_2.pth')), _load(os.path.join(plain, 'ckps', 'ckp_2.pth'))
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k
    assert np.array_equal(np.load(os.path.join(full, 'valdice.npz'))['valdice'],
                          np.load(os.path.join(plain, 'valdice.npz'))['valdice'])
    assert sorted(os.listdir(os.path.join(full, 'ckps'))) == ['ckp_2.pth', 'state_0.pth', 'state_1.pth', 'state_2.pth']


def test_resume_with_cpu_input_into_the_graph_replay(tmp_path):
    """--cpu_input --num_workers 0, resumed from state_1 with --graph_step added on resume only (the replay is bit-identical to
    the eager step)."""
    _resume_case(tmp_path, 'train_chaos.py', SMALL + FULL + ['--epoch', '3', '--cpu_input', '--num_workers', '0'], 1, 2,
                 resume_extra=['--graph_step'])


@pytest.mark.parametrize('storage,scale', [('bf16', 2.0 ** 127), ('fp16', 2.0 ** 40)])
def test_resume_carries_the_halved_loss_scale(tmp_path, storage, scale):
    """16-bit storage with an initial loss scale that overflows the scaled gradients: epoch 0 skips most optimizer steps and
    halves the scale (a numeric overflow the guard catches, nothing faults).  The halved scale and the guard's counters carry
    over into the resumed run."""
    full, copy, st = _resume_case(tmp_path, 'train_chaos.py',
                                  SMALL + FULL + ['--epoch', '3', '--storage', storage, '--num_workers', '0'], 0, 2,
                                  env={'PP_LOSS_SCALE': repr(scale)})
    s0 = _load(os.path.join(full, 'ckps', 'state_0.pth'))
    assert s0['loss_scale'] == scale / 2 and int(s0['guard'][1]) > 0 and s0['skipped_logged'] == int(s0['guard'][1])
    assert 'skipped' in open(os.path.join(copy, 'log.txt')).read()


def test_resume_with_momentum_sgd(tmp_path):
    _, _, st = _resume_case(tmp_path, 'train_chaos.py',
                            SMALL + FULL + ['--epoch', '3', '--optimizer', 'momentum', '--num_workers', '0'], 0, 2)
    assert set(st['optimizer']['slabs'][0]) == {'momentum_buffer', 'steps'}
    assert st['optimizer']['slabs'][0]['steps'] == {'backbone': 12, 'aux_path': 12}


def test_resume_the_upper_bound(tmp_path):
    _, _, st = _resume_case(tmp_path, 'upper_bound_chaos.py', SMALL + ['--epoch', '3', '--num_workers', '0'], 0, 2,
                            session='Upperbound')
    assert st['optimizer']['slabs'][0]['steps'] == {'backbone': 12}


def test_resume_two_ranks(tmp_path):
    """Two ranks through torch.distributed.run (gloo, both on one GPU, as test_gpu_parallel.py launches them): rank 0 writes every
    rank's generator states, each rank restores its own.  A resume with one rank is refused."""
    env = {'PP_DIST_BACKEND': 'gloo', 'PP_SHARE_GPU': '1', 'PP_HANG_DUMP': '240'}
    argv = SMALL + FULL + ['--epoch', '3', '--num_workers', '0']
    full, copy, st = _resume_case(tmp_path, 'train_chaos.py', argv, 0, 2, env=env, nproc=2)
    assert st['world_size'] == 2 and len(st['rng']) == 2
    assert not torch.equal(st['rng'][0]['cuda'], st['rng'][1]['cuda']) or \
        not np.array_equal(st['rng'][0]['augmenter'][1].numpy(), st['rng'][1]['augmenter'][1].numpy())
    r = _driver('train_chaos.py', argv + ['--tag', 'r', '--root', str(tmp_path / 'resumed'), '--resume', copy])
    assert r.returncode == 2 and 'world size 2' in r.stderr, r.stderr[-3000:]
