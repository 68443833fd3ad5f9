"""GPU: instance_norm_grad.hip (scf_instance_norm_grad, scf_instance_norm_res_norm_grad), RAFTEncoder.keeping /
in_backward on the InstanceNorm encoder and SCFlowRefiner.feature_grads against the float64 restatements and the derived
bound of tests/test_feature_grad_host.py.  Every launch of the new kernel is compared as `error <= bound` over ALL
elements (ratio <= 1) given its own operands, or by bit equality.  The composed gradients are held to float64 autograd of
the whole encoder, max |g - g64| / max |g64| per tensor inside FH.GOLDEN_ROOM, the biases that are 0 in exact arithmetic to
FH.ZERO_BIAS_ROOM x the layer's sum |du|, and to the reference module's fixture inside twice those (two fp32 evaluations
around one float64 value)."""
import numpy as np
import pytest
import torch

import scflow_amd
from scflow_amd import modules, ops
from scflow_amd._lib import ScflowHipError
from scflow_amd.modules import RAFTEncoder
import test_feature_grad_host as FH
import test_loss_host as HL
from test_stream_ops_host import f64, measured, same_bits, worst_ratio  # noqa: E402
from test_gpu_gru_grad import scflow_model  # noqa: F401  (the small random-weight refiner, a module-scoped fixture)

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
cpu = lambda t: t.detach().cpu()                                    # noqa: E731
GUARD = 1234.5


def D(t):
    return None if t is None else (torch.from_numpy(t) if isinstance(t, np.ndarray) else t).to(DEV).contiguous()


def run_form(case, guarded=False):
    """ops.instance_norm_grad on a host case -> dict of the kernel's outputs (GPU tensors), named as FH.in_grad64 names
    them.  ``guarded``: the destinations sit inside larger buffers filled with GUARD, which must keep their bits."""
    dev = {k: D(v) for k, v in case.items()}
    nout = 1 if 'y' not in case else 2
    out = None
    if guarded:
        n = case['g'].numel()
        bufs = [torch.full((n + 512,), GUARD, device=DEV) for _ in range(nout)]
        out = [b[256:256 + n].view(case['g'].shape) for b in bufs]
    res = ops.instance_norm_grad(dev['g'], dev['u'], y=dev.get('y'), r=dev.get('r'), out=out)
    if guarded:
        for b in bufs:
            assert bool((b[:256] == GUARD).all()) and bool((b[256 + n:] == GUARD).all()), 'a guard value was overwritten'
    if nout == 1:
        return dict(du=res)
    return dict(zip(('du', 'dr') if 'r' in case else ('gp', 'du'), res))


def check_form(case, tag, aligned=True):
    got = run_form(case, guarded=True)
    ref = FH.in_grad_ref(**case, aligned=aligned)
    assert sorted(got) == sorted(ref)
    worst = max(worst_ratio(cpu(got[k]), *ref[k]) for k in ref)
    measured(f'instance_norm_grad {tag}: worst error / bound', worst)
    return got, worst


# ============================================================================================================ kernels
@pytest.mark.parametrize('hw', FH.GRAD_SHAPES, ids=lambda v: f'{v[0]}x{v[1]}')
@pytest.mark.parametrize('form', FH.FORMS)
def test_forms_against_float64(form, hw):
    planes = 2 + (hw[0] * hw[1]) % 4                                # 2 to 5 planes
    case = FH.grad_case(form, planes, hw)
    got, worst = check_form(case, f'{form} {hw} x {planes} planes')
    assert worst <= 1.0
    assert all(bool(torch.isfinite(v).all()) for v in got.values())
    if hw == (1, 1):
        assert not bool(got['du'].any()) and ('dr' not in got or not bool(got['dr'].any()))
    if 'gp' in got:                                                 # the shortcut's cotangent: G where y > 0, +0 elsewhere
        assert same_bits(got['gp'], torch.where(D(case['y']) > 0, D(case['g']), torch.zeros((), device=DEV)))
    for _ in range(2):                                              # three runs, equal bits
        again = run_form(case)
        assert all(same_bits(again[k], got[k]) for k in got), 'two runs differ'


@pytest.mark.parametrize('form', FH.FORMS)
def test_unaligned_pointers_take_the_sweeps(form):
    """a plane count and size that would take the register form, at an address 4 bytes off a 16-byte boundary"""
    case = FH.grad_case(form, 3, (32, 32), seed=5)
    dev = {}
    for k, v in case.items():
        buf = torch.empty((v.numel() + 1,), device=DEV)
        dev[k] = buf[1:].view(v.shape)
        dev[k].copy_(v)
        assert dev[k].data_ptr() % 16 == 4
    res = ops.instance_norm_grad(dev['g'], dev['u'], y=dev.get('y'), r=dev.get('r'))
    got = dict(du=res) if 'y' not in case else dict(zip(('du', 'dr') if 'r' in case else ('gp', 'du'), res))
    ref = FH.in_grad_ref(**case, aligned=False)
    worst = max(worst_ratio(cpu(got[k]), *ref[k]) for k in ref)
    measured(f'instance_norm_grad {form} 32x32 unaligned: worst error / bound', worst)
    assert worst <= 1.0


REGIME_SHAPES = [(5, 7), (32, 32), (64, 64), (128, 128), (4, 4097)]


@pytest.mark.parametrize('hw', REGIME_SHAPES, ids=lambda v: f'{v[0]}x{v[1]}')
@pytest.mark.parametrize('form', FH.FORMS)
def test_regimes(form, hw):
    for regime in ('constant', 'offset', 'all_masked'):
        case = FH.grad_case(form, 3, hw, seed=1, regime=regime)
        got, worst = check_form(case, f'{form} {hw} {regime}')
        assert worst <= 1.0, regime
        if regime == 'all_masked':                                  # a zero cotangent gives zeros, never NaN
            assert all(not bool(v.any()) for v in got.values())
    # one NaN in g at an unmasked element of plane 1: that plane is NaN throughout, the neighbours keep their bits
    case = FH.grad_case(form, 3, hw, seed=2)
    clean = run_form(case, guarded=True)
    live = case['g'][0, 1].flatten().nonzero().flatten() if form == 'mid' else (case['y'][0, 1] > 0).flatten().nonzero().flatten()
    assert len(live), 'no unmasked element in plane 1'
    bad = dict(case, g=case['g'].clone())
    bad['g'].view(3, -1)[1, int(live[len(live) // 2])] = float('nan')
    got = run_form(bad, guarded=True)
    for k in ('du', 'dr'):
        if k in got:
            assert bool(torch.isnan(got[k][0, 1]).all()), k
            assert same_bits(got[k][0, 0], clean[k][0, 0]) and same_bits(got[k][0, 2], clean[k][0, 2]), k


@pytest.mark.parametrize('hw', [(2, 3), (9, 13), (32, 32), (64, 64), (128, 128), (4, 4097)], ids=lambda v: f'{v[0]}x{v[1]}')
@pytest.mark.parametrize('form', FH.FORMS)
def test_a_plane_alone_gives_the_bits_it_has_among_64(form, hw):
    case = FH.grad_case(form, 64, hw, seed=4)
    all64 = run_form(case)
    for p in (0, 37, 63):
        one = run_form({k: v[:, p:p + 1].contiguous() for k, v in case.items()})
        assert all(same_bits(one[k], all64[k][:, p:p + 1]) for k in all64), (p, list(all64))


def test_ops_refusals():
    g = D(FH._rand((1, 2, 4, 4), 1))
    with pytest.raises(ScflowHipError, match='must be'):
        ops.instance_norm_grad(g, g[:, :1].contiguous())
    with pytest.raises(ScflowHipError, match='comes with y'):
        ops.instance_norm_grad(g, g, r=g)
    with pytest.raises(ScflowHipError, match='destination'):
        ops.instance_norm_grad(g, g, y=g, out=[None])
    with pytest.raises(ScflowHipError):
        ops.instance_norm_grad(g.cpu(), g)
    with pytest.raises(ScflowHipError, match='contiguous'):
        ops.instance_norm_grad(g, g.transpose(2, 3))


# ============================================================================================================ the chain
def build_encoder(sd, kind='IN'):
    enc = RAFTEncoder(3, FH.OUT_CHANNELS, norm_cfg=dict(type=kind)).to(DEV)
    if sd is not None:
        enc.load_state_dict({k: v for k, v in sd.items()}, strict=True)
    return enc


def keep_forward(enc, x):
    with enc.keeping():
        y = enc(D(x))
    return y, enc.kept


KEPT_KEYS = sorted(['x', 'stem', 'u_stem', 'out', 'r2', 'r4'] + [f'{k}{i}' for i in range(6) for k in ('t', 'y', 'u1_', 'u2_')])


def in_place_forward(enc, x):
    """the InstanceNorm forward outside keeping() as the parent commit launches it: every normalisation into the
    convolution's own output, the shortcut's inside the block's final pass"""
    def block(q, y):                                                # a block's tensors live as long as the block runs
        if 'ds' in q:
            t, idt = ops.conv2d_pair((q['c1'], y), (q['ds'], y))
        else:
            t, idt = ops.conv2d(q['c1'], y), y
        ops.instance_norm(t, relu=True, out=t)
        u2 = ops.conv2d(q['c2'], t)
        return ops.instance_norm(u2, res=idt, relu=True, out=u2, res_norm='ds' in q)

    p = enc.packed
    y = ops.conv2d(p['stem'], x)
    stem = ops.instance_norm(y, relu=True, out=y)                   # the stem's output lives to the end of the forward
    for name in enc.res_layers:
        for blk in getattr(enc, name):
            y = block(blk.packed, y)
    out = ops.conv2d(p['head'], y)
    del stem
    return out


def out_of_place_forward(enc, x):
    """the InstanceNorm forward under keeping() as the parent commit launches it: the same launches with every
    normalisation out of place, a shortcut's raw output normalised in a copy -> (the head's output, what it keeps)"""
    p = enc.packed
    kept = dict(x=x, u_stem=ops.conv2d(p['stem'], x))
    y = kept['stem'] = ops.instance_norm(kept['u_stem'], relu=True)
    for i, blk in enumerate(blk for name in enc.res_layers for blk in getattr(enc, name)):
        q = blk.packed
        if 'ds' in q:
            u1, r = ops.conv2d_pair((q['c1'], y), (q['ds'], y))
            kept[f'r{i}'] = r
        else:
            u1, r = ops.conv2d(q['c1'], y), None
        t = ops.instance_norm(u1, relu=True)
        u2 = ops.conv2d(q['c2'], t)
        y = ops.instance_norm(u2, res=y if r is None else r.clone(), relu=True, res_norm=r is not None)
        kept.update({f't{i}': t, f'y{i}': y, f'u1_{i}': u1, f'u2_{i}': u2})
    kept['out'] = ops.conv2d(p['head'], y)
    return kept['out'], kept


def recorded(fn):
    """fn() -> (its result, (ran, paired, variants) of ops.record_conv_kernels around it)"""
    rec = ops.record_conv_kernels()
    with rec:
        res = fn()
    return res, (rec.ran, rec.paired, rec.variants)


def peak_over_baseline(fn):
    """the most device memory allocated during fn() over what was allocated before it"""
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    res = fn()
    torch.cuda.synchronize()
    del res
    return torch.cuda.max_memory_allocated() - base


@pytest.mark.parametrize('n', [1, 3])
@pytest.mark.parametrize('hw', [(18, 26), (16, 24)], ids=lambda v: f'{v[0]}x{v[1]}')
def test_forward_modes_launch_what_the_lists_do(hw, n):
    """the InstanceNorm encoder's two forward modes against the launch lists above: the bits of the output and of every
    kept tensor, the convolution routes, and what may alias; 18 x 26 has 3 x 4 planes at the coarsest level (HW % 4 != 0)"""
    sd = FH.encoder_params(FH.CASE_SEED)
    x = D(FH.encoder_inputs(FH.CASE_SEED, n, *hw)[0])
    enc = build_encoder(sd)
    want, routes = recorded(lambda: in_place_forward(enc, x))
    y, ran = recorded(lambda: enc(x))
    assert same_bits(y, want) and ran == routes and enc.kept == {}
    (want_k, want_kept), routes_k = recorded(lambda: out_of_place_forward(enc, x))
    (y_k, kept), ran_k = recorded(lambda: keep_forward(enc, x))
    assert same_bits(y_k, want_k) and same_bits(y_k, want) and ran_k == routes_k == routes
    assert sorted(kept) == sorted(want_kept) == KEPT_KEYS and all(same_bits(kept[k], want_kept[k]) for k in kept)
    assert sorted(kept) == sorted(modules._kept_keys(modules._RawIN, enc._blocks()))
    # keeping: no raw output shares storage with its normalised map, nor any kept tensor with another; the output is the
    # forward's own unless the caller owns its destination, then a copy
    ptrs = [v.data_ptr() for v in kept.values()]
    assert len(set(ptrs)) == len(ptrs) and kept['x'] is x and kept['out'] is y_k
    dest = torch.empty_like(want)
    with enc.keeping():
        y_d = enc(x, out=dest)
    ptrs = [v.data_ptr() for v in enc.kept.values()]
    assert y_d.data_ptr() == dest.data_ptr() and dest.data_ptr() not in ptrs and len(set(ptrs)) == len(ptrs)
    assert same_bits(enc.kept['out'], dest) and same_bits(dest, want)
    # plain: the norms write into the convolutions' own outputs, so the forward allocates no more than the list does
    del y, y_k, kept, want_k, want_kept, y_d
    enc(x)
    assert enc.kept == {}
    peak, peak_list = peak_over_baseline(lambda: enc(x)), peak_over_baseline(lambda: in_place_forward(enc, x))
    measured(f'RAFTEncoder forward {hw} N {n}, in place: peak bytes over the baseline, module / list', peak / peak_list)
    assert 0 < peak <= peak_list


def compare_composed(tag, grads, saved, x, sd, g_out, prefix=''):
    """the 32 gradients against float64 autograd of the whole encoder (this file's host graph with the GPU forward's ReLU
    decisions at units within fp32 rounding of zero) -> FH.composed_error"""
    ties = []
    acts, truth = FH.truth64(x, sd, g_out, relu=FH.relu_decisions(saved), ties=ties)
    for key, count, v in ties:
        measured(f'{tag}: ReLU units of {key} within fp32 rounding of zero and decided otherwise by the GPU forward: {count}; '
                 'worst |pre-activation| / allowed', v)
    launches = {}
    FH.backward_ref64(acts, sd, g_out, launches=launches)
    return FH.composed_error({k: cpu(grads[prefix + k]) for k in FH.PARAM_NAMES}, truth, FH.zero_bias_scales(launches)), launches


def check_launches(im):
    """every launch of the new kernel in the walk, given its own operands, against the derived bound"""
    worst = 0.0
    for key, rec in im.items():
        if not (key == 'in1' or key.endswith(('.in1', '.in2'))):
            continue
        case = {k: cpu(rec[k]) for k in ('g', 'u', 'y', 'r') if k in rec}
        ref = FH.in_grad_ref(**case)
        worst = max([worst] + [worst_ratio(cpu(rec[k]), *ref[k]) for k in ref])
    return worst


@pytest.mark.parametrize('n', [1, 4])
@pytest.mark.parametrize('hw', [(18, 26), (16, 24)], ids=lambda v: f'{v[0]}x{v[1]}')
def test_in_backward_launch_by_launch(hw, n):
    sd = FH.encoder_params(FH.CASE_SEED)
    x, g = FH.encoder_inputs(FH.CASE_SEED, n, *hw)
    enc = build_encoder(sd)
    plain = enc(D(x))
    assert enc.kept == {}, 'a forward outside keeping() keeps nothing'
    y, saved = keep_forward(enc, x)
    assert same_bits(y, plain), 'keeping changes the forward'
    assert sorted(saved) == KEPT_KEYS
    again = enc(D(x))
    assert same_bits(again, plain) and enc.kept == {}
    # the kept activations are the forward's: the normalised maps of the raw outputs, bit for bit
    assert same_bits(saved['stem'], ops.instance_norm(saved['u_stem'].clone(), relu=True))
    assert same_bits(saved['y2'], ops.instance_norm(saved['u2_2'].clone(), res=saved['r2'].clone(), relu=True, res_norm=True))
    assert same_bits(saved['y1'], ops.instance_norm(saved['u2_1'].clone(), res=saved['y0'], relu=True))
    im = {}
    grads = enc.in_backward(saved, D(g), intermediates=im)
    assert sorted(grads) == sorted(dict(enc.named_parameters())) and len(grads) == 32
    assert all(grads[k].shape == v.shape for k, v in enc.named_parameters())
    # the records come in launch order: the head, the blocks last to first (each norm in front of its convolution), the stem
    assert list(im) == ['head'] + [f'res_layer{L}.{j}.{c}' for L in (3, 2, 1) for j in (1, 0)
                                   for c in ('in2', 'conv2', 'in1', 'conv1') + (('downsample',) if j == 0 and L > 1 else ())
                                   ] + ['in1', 'conv1']
    v = check_launches(im)
    measured(f'RAFTEncoder.in_backward {hw} N {n}, the InstanceNorm launches: worst error / bound', v)
    assert v <= 1.0
    (worst, worst0), _ = compare_composed(f'{hw} N {n}', grads, saved, x, sd, g)
    measured(f'RAFTEncoder.in_backward {hw} N {n}, composed: worst max error / largest float64 entry', worst)
    measured(f'RAFTEncoder.in_backward {hw} N {n}, composed: worst |zero bias gradient| / sum |du|', worst0)
    assert worst <= FH.GOLDEN_ROOM and worst0 <= FH.ZERO_BIAS_ROOM
    # the biases in front of an InstanceNorm are computed, not hard-wired
    assert any(bool(grads[k].any()) for k in FH.ZERO_BIASES)
    # a second run: the same bits; accumulation doubles them; a prefix and foreign entries
    again = enc.in_backward(saved, D(g))
    assert all(same_bits(again[k], grads[k]) for k in grads)
    into = {k: v.clone() for k, v in grads.items()}
    assert enc.in_backward(saved, D(g), param_grads=into) is into
    assert all(same_bits(into[k], grads[k] + grads[k]) for k in grads)
    pre = {'render_encoder.' + k: v.clone() for k, v in grads.items()}
    pre['other'] = D(FH._rand((3,), 1))
    enc.in_backward(saved, D(g), param_grads=pre, prefix='render_encoder.')
    assert all(same_bits(pre['render_encoder.' + k], grads[k] + grads[k]) for k in grads) and len(pre) == 33


def test_in_backward_against_the_reference_fixture():
    z = np.load(FH.GOLDEN)
    for hw in FH.GOLDEN_SIZES:
        tag, sd, x, g = FH.golden_case(hw)
        enc = build_encoder(sd)
        _, saved = keep_forward(enc, x)
        im = {}
        grads = enc.in_backward(saved, D(g), intermediates=im)
        scales = {'conv1.bias': im['in1']['du']}
        for key, _, _, stride in FH.BLOCKS:
            scales[f'{key}.conv1.bias'], scales[f'{key}.conv2.bias'] = im[f'{key}.in1']['du'], im[f'{key}.in2']['du']
            if stride != 1:
                scales[f'{key}.downsample.0.bias'] = im[f'{key}.in2']['dr']
        worst, worst0 = 0.0, 0.0
        for name in FH.PARAM_NAMES:
            got = f64(FH.golden_pick(name, cpu(grads[name]).numpy()))
            want = f64(z[f'{tag}.{name}'])
            if name in FH.ZERO_BIASES:
                worst0 = max(worst0, float((np.abs(got - want) / f64(scales[name].abs().sum((0, 2, 3)))).max()))
            else:
                worst = max(worst, float(np.abs(got - want).max() / float(grads[name].abs().max())))
        measured(f'RAFTEncoder.in_backward against the reference module {tag}: worst max error / largest entry', worst)
        measured(f'RAFTEncoder.in_backward against the reference module {tag}: worst zero-bias difference / sum |du|', worst0)
        assert worst <= 2 * FH.GOLDEN_ROOM and worst0 <= 2 * FH.ZERO_BIAS_ROOM


def test_in_backward_errors():
    sd = FH.encoder_params(FH.CASE_SEED)
    x, g = FH.encoder_inputs(FH.CASE_SEED, 1, 16, 24)
    enc = build_encoder(sd)
    _, saved = keep_forward(enc, x)
    g = D(g)
    for key in ('x', 'stem', 'u_stem', 't3', 'y5', 'u1_0', 'u2_5', 'r2', 'r4'):
        with pytest.raises(ScflowHipError, match='keeping'):
            enc.in_backward({k: v for k, v in saved.items() if k != key}, g)
    with pytest.raises(ScflowHipError, match='keeping'):
        enc.in_backward(None, g)
    for bad in (g[:, :128], g[:, :, :1], (g[:, :128], g[:, 128:])):
        with pytest.raises(ScflowHipError, match='g_out'):
            enc.in_backward(saved, bad)
    grads = enc.in_backward(saved, g)
    with pytest.raises(ScflowHipError, match='but not all'):
        enc.in_backward(saved, g, param_grads={'conv2.bias': grads['conv2.bias']})
    ctx = build_encoder(None, kind='BN')
    with ctx.keeping():
        ctx(D(x))
    with pytest.raises(NotImplementedError, match='BatchNorm encoder'):
        ctx.in_backward(ctx.kept, g)
    quarter = RAFTEncoder(3, FH.OUT_CHANNELS, scale=1 / 4, norm_cfg=dict(type='IN')).to(DEV)
    with pytest.raises(NotImplementedError, match='stride-1 stem'):
        quarter.in_backward(saved, g)
    with pytest.raises(NotImplementedError, match='in_backward'):
        enc.backward(saved, g)
    enc(D(x))
    assert enc.kept == {} and not enc.keep


# ================================================================================================= the refiner's entry
def _get_pose(m, data):
    return m.get_pose(data['rendered_images'], data['real_images'], data['ref_rotations'], data['ref_translations'],
                      data['rendered_depths'], data['internel_k'], data['labels'])


def _same(a, b):
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    return (a is None and b is None) or same_bits(a, b)


def _feature_case(m, data, seed):
    rend, real = data['rendered_images'].contiguous(), data['real_images'].contiguous()
    plain = [t.clone() for t in m.extract_feat(rend, real)]
    shape = tuple(plain[0].shape)
    return rend, real, plain, D(FH._rand(shape, seed)), D(FH._rand(shape, seed + 1))


def test_feature_grads_shared_encoder(scflow_model):  # noqa: F811
    m, case = scflow_model
    assert m.render_encoder is m.real_encoder
    data = HL.refiner_data(case, DEV)
    before = _get_pose(m, data)
    rend, real, plain, g_rend, g_real = _feature_case(m, data, 300)
    fe = m.render_encoder
    assert fe.kept == {}
    with fe.keeping():
        feats = m.extract_feat(rend, real)
    assert all(same_bits(a, b) for a, b in zip(feats, plain)), 'keeping changes extract_feat'
    assert sorted(fe.kept) == KEPT_KEYS and fe.kept['x'].shape[0] == 2 * rend.shape[0] and m.context.kept == {}
    saved = dict(fe.kept)
    grads = m.feature_grads(g_rend, g_real)
    assert fe.kept == {} and not fe.keep
    names = [k for k, _ in m.named_parameters() if k.startswith(('render_encoder.', 'real_encoder.'))]
    assert sorted(grads) == sorted(names) and len(grads) == 32 and all(k.startswith('render_encoder.') for k in grads)
    # one pass over the 2N stacked cotangents: in_backward on the stacked batch, bit for bit
    stage = fe.in_backward(saved, torch.cat((g_rend, g_real)), prefix='render_encoder.')
    assert all(same_bits(stage[k], grads[k]) for k in grads)
    # accumulated into a dict that already holds them
    with fe.keeping():
        m.extract_feat(rend, real)
    into = {k: v.clone() for k, v in grads.items()}
    assert m.feature_grads(g_rend, g_real, param_grads=into) is into
    assert all(same_bits(into[k], grads[k] + grads[k]) for k in grads)
    # refusals by name: nothing kept; cotangents of the wrong shape (what was kept is dropped all the same)
    with pytest.raises(ScflowHipError, match='keeping'):
        m.feature_grads(g_rend, g_real)
    with fe.keeping():
        m.extract_feat(rend, real)
    with pytest.raises(ScflowHipError, match='g_out'):
        m.feature_grads(g_rend[:, :, :1], g_real[:, :, :1])
    assert fe.kept == {}
    with pytest.raises(ScflowHipError, match='one shape'):
        m.feature_grads(g_rend, g_real[:1, :, :1])
    # plain calls before and after: the same bits, nothing kept
    assert _same(list(before), list(_get_pose(m, data)))
    assert fe.kept == {} and m.context.kept == {}
    # nothing joins the feature encoder to the training step yet
    assert not any(k.startswith(('render_encoder.', 'real_encoder.')) for k, _ in m.trainable_parameters())


def test_feature_grads_separate_encoders(scflow_model):  # noqa: F811
    _, case = scflow_model
    cfg = scflow_amd.scflow_model_cfg(iters=HL.REFINER_ITERS)
    cfg['seperate_encoder'] = True
    torch.manual_seed(11)
    m = scflow_amd.build_refiner(cfg).to(DEV)
    assert m.render_encoder is not m.real_encoder
    data = HL.refiner_data(case, DEV)
    rend, real, plain, g_rend, g_real = _feature_case(m, data, 400)
    fe, re_ = m.render_encoder, m.real_encoder
    with fe.keeping(), re_.keeping():
        feats = m.extract_feat(rend, real)
    assert all(same_bits(a, b) for a, b in zip(feats, plain)), 'keeping changes extract_feat'
    saved_f, saved_r = dict(fe.kept), dict(re_.kept)
    assert sorted(saved_f) == KEPT_KEYS and sorted(saved_r) == KEPT_KEYS
    grads = m.feature_grads(g_rend, g_real)
    assert fe.kept == {} and re_.kept == {}
    names = [k for k, _ in m.named_parameters() if k.startswith(('render_encoder.', 'real_encoder.'))]
    assert sorted(grads) == sorted(names) and len(grads) == 64
    a = fe.in_backward(saved_f, g_rend, prefix='render_encoder.')
    b = re_.in_backward(saved_r, g_real, prefix='real_encoder.')
    assert all(same_bits(grads[k], v) for k, v in {**a, **b}.items())
    assert all(same_bits(x, y) for x, y in zip(m.extract_feat(rend, real), plain)) and fe.kept == {} and re_.kept == {}
