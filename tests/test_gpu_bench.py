"""bench.py on the GPU box: `--steps` is the number of timed steps, and `--dump-outputs` writes what the last of them computed."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {'segmentation_logits', 'loss_pce', 'loss_ent', 'loss_cr', 'segmentation_logits_strong', 'logits_aux_cls', 'loss_aux_cls',
         'loss_memory', 'loss', 'parameters', 'gradients', 'buffers'}


def _bench(out_dir, steps, warmup):
    env = {k: v for k, v in os.environ.items() if k not in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'PP_FORCE_DIST', 'PP_SHARE_GPU')}
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', str(steps), '--warmup', str(warmup),
                        '--batch', '2', '--size', '64', '--no-cpu-baseline', '--no-bn-eval', '--dump-outputs', str(out_dir)],
                       env=env, cwd=ROOT, capture_output=True, text=True, timeout=280)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return json.loads([l for l in r.stdout.splitlines() if l.startswith('{')][-1])


def test_bench_steps_and_dump_outputs(tmp_path):
    """Three training iterations either way -- 1 warm-up + 2 timed, or 2 warm-ups + 1 timed -- leave the same state behind, and
    the dump of the last timed step says so; the line times exactly --steps steps."""
    ja = _bench(tmp_path / 'a', steps=2, warmup=1)
    jb = _bench(tmp_path / 'b', steps=1, warmup=2)
    for j, steps in ((ja, 2), (jb, 1)):
        assert j['steps'] == steps and len(j['step_ms']['all']) == steps and j['ms_per_step'] > 0
        assert set(j['dump_outputs']['files']) == NAMES and j['dump_outputs']['bytes'] <= 64 << 20
    for name in sorted(NAMES):
        a, b = np.load(tmp_path / 'a' / f'{name}.npy'), np.load(tmp_path / 'b' / f'{name}.npy')
        assert a.dtype == np.float32 and a.shape == b.shape and np.isfinite(a).all(), name
        assert np.allclose(a, b, rtol=1e-5, atol=1e-6 * max(1.0, float(np.abs(b).max()))), name
    loss = float(np.load(tmp_path / 'a' / 'loss.npy'))
    assert abs(loss - ja['final_loss']) <= 1e-5 * max(1.0, abs(loss))
    assert np.load(tmp_path / 'a' / 'segmentation_logits.npy').shape == (2, 5, 64, 64)
