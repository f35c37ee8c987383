"""Fine-tuning without a GPU: the --freeze_encoder / --init_from / --init_reset_head flags of both drivers, ``freeze_encoder`` on
CPU-built models, ``finetune.load_pretrained``, gradient buckets that freezing left empty (two gloo ranks), and the resume rules
for the three flags."""
import os
import socket
from types import SimpleNamespace

import pytest
import torch
import torch.multiprocessing as mp
import torch.nn as nn

from oracle import pacing_oracle as O


def _args(**over):
    return O.default_args(init_ch=4, max_ch=32, hid_ch=8, feat_ch=[32, 32], do_loss_ent=True, do_decoder_consistency=True,
                          do_aux_path=True, do_memory=True, **over)


def _unet(num_classes=5, **kw):
    from pacingpseudo_amd.models import UNet
    return UNet(input_ch=1, init_ch=4, max_ch=32, num_classes=num_classes, output_stride=8, elab_end_points=True, **kw)


def _full(num_classes=5, **kw):
    from pacingpseudo_amd.models import ConsistencyRegulr
    a = _args(num_classes=num_classes, ignored_index=num_classes)
    return ConsistencyRegulr(
        kwargs_unet=dict(input_ch=1, init_ch=4, max_ch=32, num_classes=num_classes, output_stride=8, is_stride_conv=False,
                         is_trans_conv=False, elab_end_points=True, **kw),
        kwargs_aux_path=dict(num_classes=num_classes, feat_stage=a.feat_stage, feat_ch=a.feat_ch, hid_ch=8, aux_drop_prob=0.0,
                             do_memory=True, max_step=400, update_momentum=0.9, ensemble_mode='cosine_similarity'),
        args_parser=a)


def _parsers():
    from pacingpseudo_amd.train import parser as p1
    from pacingpseudo_amd.upper_bound import parser as p2
    return [p1, p2]


# ---------------------------------------------------------------------------------------------------------------- flags
@pytest.mark.parametrize('which', [0, 1])
def test_flags_defaults_and_refusals(which, capsys):
    parser = _parsers()[which]
    ns = parser.parse_args(['--tag', 't'])
    assert (ns.freeze_encoder, ns.init_from, ns.init_reset_head) == (0, None, False)
    ns = parser.parse_args(['--tag', 't', '--freeze_encoder', '6', '--init_from', 'a.pth', '--init_reset_head'])
    assert (ns.freeze_encoder, ns.init_from, ns.init_reset_head) == (6, 'a.pth', True)
    for bad in ('-1', '7', 'x'):
        with pytest.raises(SystemExit) as e:
            parser.parse_args(['--tag', 't', '--freeze_encoder', bad])
        assert e.value.code == 2
        assert '--freeze_encoder' in capsys.readouterr().err


# ---------------------------------------------------------------------------------------------------------------- freeze_encoder
def _frozen_names(model):
    return [n for n, p in model.named_parameters() if not p.requires_grad and not n.endswith('memory_bank')]


@pytest.mark.parametrize('kind', ['unet', 'full'])
def test_freeze_encoder_partitions_the_parameters(kind):
    model = _unet() if kind == 'unet' else _full()
    bb = model if kind == 'unet' else model.backbone
    pre = '' if kind == 'unet' else 'backbone.'
    keys = list(model.state_dict())
    assert bb.frozen_stages == 0 and _frozen_names(model) == []
    for n in (3, 6, 1, 0):                                   # each call re-partitions
        assert model.freeze_encoder(n) is model
        assert bb.frozen_stages == n
        want = [k for k, _ in model.named_parameters() if any(k.startswith(f'{pre}enc_block{s}.') for s in range(1, n + 1))]
        assert _frozen_names(model) == want and len(want) == 8 * n
        assert all(p.grad is None for p in model.parameters())
        # train() leaves the frozen stages' norm modules in eval mode; eval() and train() again keep that
        for mode in (True, False, True):
            model.train(mode)
            for s in range(1, 7):
                for m in getattr(bb, f'enc_block{s}').modules():
                    if isinstance(m, nn.BatchNorm2d):
                        assert m.training == (mode and s > n), (n, s, mode)
            assert bb.dec_block3.conv_block.conv_layer1.norm_op.training == mode
            assert bb.training == mode
    assert list(model.state_dict()) == keys
    for bad in (-1, 7, 2.0, '3', None, True):
        with pytest.raises(ValueError, match='0 .. 6'):
            model.freeze_encoder(bad)
    assert bb.frozen_stages == 0


def test_freeze_encoder_with_groupnorm_blocks_keeps_the_keys():
    model = _unet(norm_op='group', norm_groups=4)
    keys = list(model.state_dict())
    model.freeze_encoder(2).train()
    assert not model.enc_block2.conv_block.conv_layer2.norm_op.training and model.enc_block3.conv_block.conv_layer1.norm_op.training
    assert list(model.state_dict()) == keys and len(_frozen_names(model)) == 16


def test_engine_refuses_anything_but_a_prefix():
    """Checked on the host before any launch: a stray requires_grad_(False), a hole in the prefix, a thawed parameter inside it."""
    model = _full()
    eng = model.engine
    assert eng._frozen_stages() == 0
    model.backbone.dec_block2.conv_block.conv_layer1.conv.weight.requires_grad_(False)
    with pytest.raises(NotImplementedError, match='backbone.dec_block2.conv_block.conv_layer1.conv.weight'):
        eng._frozen_stages()
    model.freeze_encoder(3)
    assert eng._frozen_stages() == 3
    model.backbone.enc_block2.conv_block.conv_layer2.norm_op.bias.requires_grad_(True)
    with pytest.raises(NotImplementedError, match='backbone.enc_block2.conv_block.conv_layer2.norm_op.bias'):
        eng._frozen_stages()
    model.freeze_encoder(3)
    model.backbone.enc_block5.conv_block.conv_layer1.conv.bias.requires_grad_(False)
    with pytest.raises(NotImplementedError, match='enc_block5'):
        eng._frozen_stages()


# ---------------------------------------------------------------------------------------------------------------- load_pretrained
def _randomise(model, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for v in model.state_dict().values():
            if v.is_floating_point():
                v.copy_(torch.rand(v.shape, generator=g) + 0.5)
            else:
                v.fill_(seed)
    return {k: v.detach().clone() for k, v in model.state_dict().items()}


@pytest.mark.parametrize('src_kind', ['unet', 'full'])
@pytest.mark.parametrize('dst_kind', ['unet', 'full'])
def test_load_pretrained_both_layouts_into_both_kinds(src_kind, dst_kind):
    from pacingpseudo_amd.finetune import load_pretrained
    ck = _randomise(_unet() if src_kind == 'unet' else _full(), 3)
    torch.manual_seed(7)
    dst = _unet() if dst_kind == 'unet' else _full()
    fresh = {k: v.detach().clone() for k, v in dst.state_dict().items()}
    loaded, reset, absent = load_pretrained(dst, ck)
    got = dst.state_dict()
    assert reset == []
    assert sorted(loaded + absent) == sorted(got) and not set(loaded) & set(absent)
    # a checkpoint without aux_path. keys leaves the auxiliary path at its fresh initialisation
    assert absent == ([k for k in got if k.startswith('aux_path.')] if (dst_kind == 'full' and src_kind == 'unet') else [])
    for k in loaded:
        sk = k
        if src_kind != dst_kind and k.startswith('backbone.'):
            sk = k[len('backbone.'):]
        elif src_kind != dst_kind:
            sk = 'backbone.' + k
        assert torch.equal(got[k], ck[sk]), k
    for k in absent:
        assert torch.equal(got[k], fresh[k]), k


@pytest.mark.parametrize('dst_kind', ['unet', 'full'])
def test_load_pretrained_head_of_another_class_count(dst_kind):
    from pacingpseudo_amd.finetune import HEAD_KEYS, load_pretrained
    ck = _randomise(_full(num_classes=3), 5)
    torch.manual_seed(9)
    dst = _unet() if dst_kind == 'unet' else _full()
    fresh = {k: v.detach().clone() for k, v in dst.state_dict().items()}
    with pytest.raises(ValueError, match='--init_reset_head'):
        load_pretrained(dst, ck)
    for k, v in dst.state_dict().items():
        assert torch.equal(v, fresh[k]), k                 # a refused checkpoint changes nothing
    loaded, reset, absent = load_pretrained(dst, ck, reset_head=True)
    pre = '' if dst_kind == 'full' else 'backbone.'
    want_reset = [k for k in dst.state_dict() if pre + k in HEAD_KEYS]
    assert sorted(reset) == sorted(want_reset) and len(reset) == (4 if dst_kind == 'full' else 2) and absent == []
    for k, v in dst.state_dict().items():
        if k in reset:
            assert torch.equal(v, fresh[k]), k
        else:
            assert torch.equal(v, ck[k if dst_kind == 'full' else 'backbone.' + k]), k
    # same class count + reset_head: the head is kept fresh all the same
    ck5 = _randomise(_full(), 6)
    dst2 = _full()
    f2 = {k: v.detach().clone() for k, v in dst2.state_dict().items()}
    _, reset2, _ = load_pretrained(dst2, ck5, reset_head=True)
    assert sorted(reset2) == sorted(HEAD_KEYS)
    assert all(torch.equal(dst2.state_dict()[k], f2[k]) for k in HEAD_KEYS)


def test_load_pretrained_refuses_what_does_not_fit():
    from pacingpseudo_amd.finetune import load_pretrained
    from pacingpseudo_amd.models import UNet
    gn = _randomise(_unet(norm_op='group', norm_groups=4), 1)
    with pytest.raises(ValueError, match='--norm_op group'):
        load_pretrained(_full(), gn)
    bn = _randomise(_unet(), 1)
    with pytest.raises(ValueError, match='--norm_op batch'):
        load_pretrained(_unet(norm_op='group', norm_groups=4), bn)
    wide = _randomise(UNet(input_ch=1, init_ch=8, max_ch=32, num_classes=5, output_stride=8), 1)
    with pytest.raises(ValueError, match='--init_ch'):
        load_pretrained(_unet(), wide)
    part = {k: v for k, v in bn.items() if not k.startswith('enc_block4.')}
    with pytest.raises(ValueError, match='enc_block4'):
        load_pretrained(_full(), part)
    with pytest.raises(ValueError, match='does not have'):
        load_pretrained(_unet(), dict(bn, **{'dec_block3.up_samp.weight': torch.zeros(2, 2, 2, 2)}))


def test_driver_init_is_a_usage_error_or_a_log_line(tmp_path):
    """finetune.init_model: a head mismatch leaves through parser.error (status 2) with the flag named; under --resume the file is
    not even opened; the three key lists reach the log."""
    from pacingpseudo_amd import finetune
    from pacingpseudo_amd.train import parser
    path = str(tmp_path / 'k3.pth')
    torch.save(_randomise(_full(num_classes=3), 2), path)
    lines = []
    with pytest.raises(SystemExit) as e:
        finetune.init_model(SimpleNamespace(init_from=path, init_reset_head=False, resume=None, freeze_encoder=0), _full(), parser, lines.append)
    assert e.value.code == 2
    with pytest.raises(SystemExit):
        finetune.init_model(SimpleNamespace(init_from=str(tmp_path / 'none.pth'), init_reset_head=False, resume=None, freeze_encoder=0),
                            _full(), parser, lines.append)
    model = _full()
    finetune.init_model(SimpleNamespace(init_from=path, init_reset_head=True, resume=None, freeze_encoder=2), model, parser, lines.append)
    assert model.backbone.frozen_stages == 2 and any('kept fresh' in s and 'memory_bank' in s for s in lines)
    assert any('--freeze_encoder 2' in s for s in lines)
    lines.clear()
    model = _full()
    finetune.init_model(SimpleNamespace(init_from='/nowhere/x.pth', init_reset_head=False, resume='run', freeze_encoder=0), model, parser, lines.append)
    assert len(lines) == 1 and 'ignored' in lines[0] and model.backbone.frozen_stages == 0


# ---------------------------------------------------------------------------------------------------------------- buckets
@pytest.mark.parametrize('n,empty', [(0, []), (3, []), (4, ['enc_rest']), (5, ['enc_rest', 'enc5']), (6, ['enc_rest', 'enc5', 'enc6'])])
def test_frozen_stages_leave_empty_buckets(n, empty):
    from pacingpseudo_amd import parallel
    from pacingpseudo_amd.flat import FlatSlab
    from tests._bucket_probe import tiling_errors
    model = _full().freeze_encoder(n)
    buckets = parallel.backbone_buckets(model)
    assert sorted(t for t, ps in buckets if not ps) == sorted(empty)
    flat = FlatSlab([('backbone', [p for p in model.backbone.parameters() if p.requires_grad]),
                     ('aux_path', [p for p in model.aux_path.parameters() if p.requires_grad])])
    red = parallel.GradReducer(model, None)
    ranges = {t: red._range(flat, t) for t, _ in buckets}
    assert sorted(t for t, r in ranges.items() if r is None) == sorted(empty)
    assert tiling_errors(flat, {t: r for t, r in ranges.items() if r is not None}, ['backbone', 'aux_path']) == []
    for t in empty:                                          # announced all the same: nothing is queued, nothing raises
        red.bucket_ready(flat, t)
    assert red.pending == []


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    torch.set_num_threads(2)
    import torch.distributed as dist
    from pacingpseudo_amd import parallel
    from pacingpseudo_amd.flat import FlatSlab
    parallel.init_from_env('gloo')
    comm = parallel.Comm()
    worst = 0.0
    for n in (4, 6):
        torch.manual_seed(1)
        model = _full().freeze_encoder(n)
        flat = FlatSlab([('backbone', [p for p in model.backbone.parameters() if p.requires_grad]),
                         ('aux_path', [p for p in model.aux_path.parameters() if p.requires_grad])])
        red = parallel.GradReducer(model, comm)
        base = torch.arange(flat.numel, dtype=torch.float32) % 251 + 1.0
        flat.grads.copy_(base * (rank + 1))
        for tag, _ in parallel.backbone_buckets(model):      # the engine's order; the empty ones included
            red.bucket_ready(flat, tag)
        assert len(red.pending) == 6 - {4: 1, 6: 3}[n]
        red.reduce(flat, ['backbone', 'aux_path'])
        assert red.pending == []
        want = base * 3.0
        for p, o in flat.offsets.items():                    # every parameter of the slab, summed exactly once
            worst = max(worst, float((flat.grads[o:o + p.numel()] - want[o:o + p.numel()]).abs().max()))
    # the epoch-0 averaging of the running statistics leaves a frozen stage's buffers alone (here: what each rank put there)
    model = _full().freeze_encoder(1)
    model.train()
    held, live = model.backbone.enc_block1.conv_block.conv_layer2.norm_op, model.backbone.enc_block2.conv_block.conv_layer1.norm_op
    with torch.no_grad():
        for bn in (held, live):
            bn.running_mean.fill_(float(rank + 1))
            bn.num_batches_tracked.fill_(7 + rank)
    parallel.sync_bn_buffers(model)
    assert torch.equal(held.running_mean, torch.full_like(held.running_mean, float(rank + 1))) and int(held.num_batches_tracked) == 7 + rank
    assert torch.equal(live.running_mean, torch.full_like(live.running_mean, 1.5)) and int(live.num_batches_tracked) == 7
    if rank == 0:
        q.put(('worst', worst))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(600)
def test_two_gloo_ranks_reduce_a_slab_with_empty_buckets():
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(540)
        assert p.exitcode == 0, f'rank process failed with exit code {p.exitcode}'
    name, worst = q.get(timeout=5)
    assert name == 'worst' and worst == 0.0


# ---------------------------------------------------------------------------------------------------------------- resume
def test_resume_rules_for_the_three_flags():
    from pacingpseudo_amd import resume
    from pacingpseudo_amd.train import apply_dataset_preset, parser
    assert resume.ABSENT_DEFAULTS['freeze_encoder'] == 0 and 'freeze_encoder' not in resume.MAY_DIFFER
    assert resume.ABSENT_DEFAULTS['init_from'] is None and resume.ABSENT_DEFAULTS['init_reset_head'] is False
    assert {'init_from', 'init_reset_head'} <= resume.MAY_DIFFER

    def flags(*extra):
        return resume.flag_dict(apply_dataset_preset(parser.parse_args(['--tag', 't', *extra])))
    new = flags()
    old = {k: v for k, v in new.items() if k not in ('freeze_encoder', 'init_from', 'init_reset_head')}
    resume.check_compatible(old, new, 1, 1)                  # a state file older than the flags resumes with the defaults
    with pytest.raises(resume.ResumeError, match='--freeze_encoder'):
        resume.check_compatible(old, flags('--freeze_encoder', '2'), 1, 1)
    with pytest.raises(resume.ResumeError, match=r'--freeze_encoder \(saved 2, now 3\)'):
        resume.check_compatible(flags('--freeze_encoder', '2'), flags('--freeze_encoder', '3'), 1, 1)
    resume.check_compatible(flags('--freeze_encoder', '2'), flags('--freeze_encoder', '2'), 1, 1)
    resume.check_compatible(flags('--init_from', 'a.pth'), flags('--init_from', 'b.pth', '--init_reset_head'), 1, 1)
    resume.check_compatible(old, flags('--init_from', 'b.pth'), 1, 1)
