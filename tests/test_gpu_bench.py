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


def _line(*args):
    """Run bench.py on one GPU at batch 2, 64x64 and return its JSON line."""
    env = {k: v for k, v in os.environ.items() if k not in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'PP_FORCE_DIST', 'PP_SHARE_GPU')}
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--batch', '2', '--size', '64'] + list(args),
                       env=env, cwd=ROOT, capture_output=True, text=True, timeout=280)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith('{')]
    assert len(lines) == 1
    return json.loads(lines[0])


def _bench(out_dir, steps, warmup):
    return _line('--steps', str(steps), '--warmup', str(warmup), '--no-cpu-baseline', '--no-bn-eval', '--dump-outputs', str(out_dir))


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


LEGS = ('bn_eval', 'mixed_precision', 'storage_fp16', 'storage_bf16', 'graph_replay', 'control')


def test_bench_plain_run_is_the_headline_and_full_adds_the_rest():
    """A plain run times the same steps as --full and stops there: no untimed profile steps (`kernels`, single-stream table,
    families outside the timed region), no extra legs, no CPU baseline.  --full still runs every leg."""
    plain = _line('--steps', '2', '--warmup', '1')
    full = _line('--steps', '2', '--warmup', '1', '--full', '--no-cpu-baseline')
    for j in (plain, full):
        assert j['metric'] == 'training images/sec (256x256, 5-class)' and j['unit'] == 'images/sec' and j['higher_is_better'] is True
        assert j['value'] > 0 and j['ms_per_step'] > 0 and j['dtype'].startswith('f32') and len(j['step_ms']['all']) == 2
    assert abs(plain['final_loss'] - full['final_loss']) <= 1e-5 * max(1.0, abs(full['final_loss']))
    roof = plain['roofline']
    assert [r['family'] for r in roof['matrix_families']] == roof['timed_by_events_in_timed_region'] and roof['achieved'] > 0
    assert plain['kernels'] is None and roof['single_stream'] is None and 'cpu_baseline' not in plain
    assert all(plain[k] is None for k in LEGS) and plain['input_pipeline_images_per_sec'] is None
    assert full['kernels'] and full['roofline']['single_stream']
    assert {r['family'] for r in roof['matrix_families']} <= {r['family'] for r in full['roofline']['matrix_families']}
    for k in LEGS:
        assert full[k] and 'error' not in full[k], (k, full[k])
    assert full['input_pipeline_images_per_sec'] > 0 and 'cpu_baseline' not in full
