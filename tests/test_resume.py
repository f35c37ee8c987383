"""--state_interval / --resume on the host: flags, the compatibility check, refused files, the directory form, the scalar-log
truncation and the atomic write (pacingpseudo_amd/resume.py).  No GPU: every refusal happens before the device is touched."""
import json
import os

import pytest
import torch

from pacingpseudo_amd import resume


def _args(parser, extra=()):
    from pacingpseudo_amd.train import apply_dataset_preset
    return apply_dataset_preset(parser.parse_args(['--tag', 't'] + list(extra)))


def _state(args, epoch=0, world=1):
    """A minimal state file of the current format (what the checks before the GPU look at)."""
    return dict(format=resume.FORMAT, version=resume.VERSION, args=resume.flag_dict(args), world_size=world, epoch=epoch)


def _write_run(tmp_path, args, epochs, world=1):
    run = tmp_path / 'run'
    (run / 'ckps').mkdir(parents=True)
    for e in epochs:
        resume.atomic_save(_state(args, e, world), resume.state_path(str(run), e))
    return run


@pytest.mark.parametrize('driver', ['train', 'upper_bound'])
def test_flags_parse_on_both_drivers(driver):
    import importlib
    parser = importlib.import_module(f'pacingpseudo_amd.{driver}').parser
    ns = parser.parse_args(['--tag', 't'])
    assert ns.state_interval == 0 and ns.resume is None
    ns = parser.parse_args(['--tag', 't', '--state_interval', '5', '--resume', 'some/run'])
    assert ns.state_interval == 5 and ns.resume == 'some/run'


@pytest.mark.parametrize('flag,value', [('--lr', '0.001'), ('--epoch', '7'), ('--storage', 'bf16')])
def test_a_flag_that_changes_the_run_is_refused_and_named(flag, value):
    from pacingpseudo_amd.train import parser
    saved = resume.flag_dict(_args(parser))
    new = resume.flag_dict(_args(parser, [flag, value]))
    with pytest.raises(resume.ResumeError) as e:
        resume.check_compatible(saved, new, 1, 1)
    assert flag in str(e.value)


def test_every_differing_flag_is_named():
    from pacingpseudo_amd.train import parser
    saved = resume.flag_dict(_args(parser))
    new = resume.flag_dict(_args(parser, ['--lr', '0.001', '--seed', '3', '--norm_op', 'group']))
    with pytest.raises(resume.ResumeError) as e:
        resume.check_compatible(saved, new, 1, 1)
    for flag in ('--lr', '--seed', '--norm_op'):
        assert flag in str(e.value)
    assert '--epoch' not in str(e.value)


def test_host_side_flags_may_differ():
    from pacingpseudo_amd.train import parser
    saved = resume.flag_dict(_args(parser, ['--state_interval', '1']))
    new = resume.flag_dict(_args(parser, ['--num_workers', '0', '--graph_step', '--gpu', '3', '--resume', 'x',
                                          '--root', 'elsewhere']))
    resume.check_compatible(saved, new, 1, 1)


def test_a_world_size_mismatch_is_refused():
    from pacingpseudo_amd.train import parser
    flags = resume.flag_dict(_args(parser))
    with pytest.raises(resume.ResumeError, match='world size 2.*world size 1'):
        resume.check_compatible(flags, flags, 1, 2)


def test_the_cli_refuses_a_world_size_mismatch_before_the_gpu(tmp_path, monkeypatch, capsys):
    from pacingpseudo_amd.train import parser, train_main
    run = _write_run(tmp_path, _args(parser), [0], world=2)
    monkeypatch.delenv('WORLD_SIZE', raising=False)
    with pytest.raises(SystemExit) as e:
        train_main(['--tag', 't', '--resume', str(run)])
    assert e.value.code == 2
    assert 'world size 2' in capsys.readouterr().err


def test_the_cli_names_a_differing_flag(tmp_path, capsys):
    from pacingpseudo_amd.upper_bound import parser, train_main
    from pacingpseudo_amd.train import apply_dataset_preset
    run = _write_run(tmp_path, apply_dataset_preset(parser.parse_args(['--tag', 't'])), [0])
    with pytest.raises(SystemExit) as e:
        train_main(['--tag', 't', '--lr', '0.5', '--resume', str(run)])
    assert e.value.code == 2
    assert '--lr' in capsys.readouterr().err


def test_a_truncated_state_file_is_refused(tmp_path, capsys):
    from pacingpseudo_amd.train import parser, train_main
    run = _write_run(tmp_path, _args(parser), [0])
    path = resume.state_path(str(run), 0)
    blob = open(path, 'rb').read()
    with open(path, 'wb') as f:
        f.write(blob[:len(blob) // 2])
    with pytest.raises(resume.ResumeError, match='not a readable run-state file'):
        resume.load(path)
    with pytest.raises(SystemExit):
        train_main(['--tag', 't', '--resume', path])
    err = capsys.readouterr().err
    assert 'not a readable run-state file' in err and 'Traceback' not in err


def test_a_weights_checkpoint_is_refused(tmp_path):
    path = str(tmp_path / 'ckp_3.pth')
    torch.save({'backbone.final_conv.weight': torch.zeros(2, 2)}, path)
    with pytest.raises(resume.ResumeError, match='not a run-state file'):
        resume.load(path)


def test_an_unknown_format_version_is_refused(tmp_path):
    from pacingpseudo_amd.train import parser
    st = _state(_args(parser))
    st['version'] = resume.VERSION + 1
    path = str(tmp_path / 'state_0.pth')
    torch.save(st, path)
    with pytest.raises(resume.ResumeError, match='unknown state format version'):
        resume.load(path)


def test_a_run_directory_resumes_from_its_highest_state(tmp_path):
    from pacingpseudo_amd.train import parser
    run = _write_run(tmp_path, _args(parser), [0, 2, 10, 9])
    (run / 'ckps' / 'state_11.pth.bak').write_text('')
    torch.save({}, str(run / 'ckps' / 'ckp_12.pth'))
    path = resume.resolve(str(run))
    assert os.path.basename(path) == 'state_10.pth'
    assert resume.run_dir_of(path) == os.path.abspath(str(run))
    assert resume.resolve(resume.state_path(str(run), 2)) == resume.state_path(str(run), 2)


def test_a_directory_without_state_is_refused(tmp_path):
    (tmp_path / 'ckps').mkdir()
    with pytest.raises(resume.ResumeError, match='no ckps/state_'):
        resume.resolve(str(tmp_path))
    with pytest.raises(resume.ResumeError, match='no such state file'):
        resume.resolve(str(tmp_path / 'missing.pth'))


def test_scalar_log_truncation_keeps_the_completed_epochs(tmp_path):
    path = tmp_path / 'scalars.jsonl'
    lines = [json.dumps(dict(tag=f'tag{i % 3}', value=float(i), step=s)) for i, s in enumerate([0, 0, 1, 1, 2, 2, 3, 1])]
    path.write_text('\n'.join(lines) + '\n' + '{"tag": "DSC/All", "val')          # a line the killed run did not finish
    resume.truncate_scalars(str(path), 1)
    kept = [json.loads(l) for l in path.read_text().splitlines()]
    assert [r['step'] for r in kept] == [0, 0, 1, 1, 1]
    assert [r['value'] for r in kept] == [0.0, 1.0, 2.0, 3.0, 7.0]
    assert sorted(os.listdir(tmp_path)) == ['scalars.jsonl']


def test_the_atomic_write_leaves_no_temporary_file(tmp_path):
    path = str(tmp_path / 'state_0.pth')
    resume.atomic_save({'a': torch.arange(3)}, path)
    resume.atomic_save({'a': torch.arange(4)}, path)                  # replaces the earlier file
    assert os.listdir(tmp_path) == ['state_0.pth']
    assert torch.equal(torch.load(path)['a'], torch.arange(4))

    class Unpicklable:
        def __reduce__(self):
            raise RuntimeError('cannot pickle')
    with pytest.raises(RuntimeError):
        resume.atomic_save({'x': Unpicklable()}, str(tmp_path / 'state_1.pth'))
    assert os.listdir(tmp_path) == ['state_0.pth']                  # a failed write leaves neither a file nor its temporary


def test_generator_states_round_trip_through_a_weights_only_file(tmp_path):
    import random
    import numpy as np
    rs = np.random.RandomState(5)
    rs.uniform(size=3)
    st = dict(python=random.getstate(), numpy=resume._np_state_out(np.random.get_state()),
              augmenter=resume._np_state_out(rs.get_state()))
    path = str(tmp_path / 's.pth')
    resume.atomic_save(st, path)
    back = torch.load(path, weights_only=True)
    expect = rs.uniform(size=4)
    rs2 = np.random.RandomState(0)
    rs2.set_state(resume._np_state_in(back['augmenter']))
    assert np.array_equal(rs2.uniform(size=4), expect)
    random.setstate(back['python'])
