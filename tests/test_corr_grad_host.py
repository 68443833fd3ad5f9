"""CPU: the adjoint of the correlation build with respect to its two feature maps (corr_build_grad.hip,
``ops.corr_build_grad``, ``SCFlowDecoder.corr_backward``) and the join it closes (``SCFlowRefiner.loss_and_network_grads``).

With level0[n][i][j] = s sum_c f1[n][c][i] f2[n][c][j], s = 1/sqrt(C), and G = d loss / d level0:

    g_f1[n][c][i] = s sum_j G[n][i][j] f2[n][c][j]          g_f2[n][c][j] = s sum_i G[n][i][j] f1[n][c][i]

`corr_build_grad64` states the two formulas in float64.  **The bound** (as DESIGN.md 4.2 derives the forward's).  The
kernel has ONE route: per output one fused-multiply-add chain from +0 over the contraction ascending (K = hw terms; the
zero steps that pad the last chunk of 32 add exact +0 products), then the scale once.  A chain of K fused multiply-adds
rounds K times, and K roundings of a recursive sum are within K U sum |G| |f| of the exact sum with no higher-order term
(Jeannerod and Rump, 2013).  The scale: sqrt(C) a power of two -> a multiplication by a power of two, exact, c0 = 0;
otherwise sqrtf(C) (one rounding of the root) and a correctly rounded division (one more), c0 = 2.  There are no chunk
combines: the accumulator runs through the chunks.  Per element, with U = 2^-24:

    |computed - exact| <= (K + c0) U s sum |G| |f|

An fp32 torch evaluation rounds no more often: `einsum` / `matmul` round K times in whatever order (K products and K - 1
sums, or K fused steps) and divide by the rounded root (exact for a power of two, two roundings else); autograd through
`oracle.correlation_pyramid` divides G by sqrt(C) first (exact, or root and division: two roundings) and contracts then.
`test_fp32_references_are_inside_the_bound` holds both to it.

**The join.**  `chain_ref64` of tests/test_chain_grad_host.py (imported; it stops at the volume) is ONE float64 graph
from the two feature maps through oracle.scflow_decoder and the loss wiring; `feature_leaves` has its own grad call return
the gradients at those two leaves as well.  Its `correlation` carried through `corr_build_grad64` must equal them to 1e-12
of their largest entry -- the stage is linear, nothing else may differ.  `ROOM` of the new `features` and `render_encoder` groups is
measured the chain test's way, against tests/golden/network_grads.npz (make_golden_network_grad.py: the reference's own
fp32 CPU `.backward()`), written down here and held to 1.5 x; the GPU tests take 2 x against float64 and 3 x against the
fixture, five times below every planted join defect (10 x room)."""
import os
from functools import lru_cache

import numpy as np
import pytest
import torch

import oracle
import test_chain_grad_host as CH
import test_loss_host as H
from test_stream_ops_host import f64, measured, worst_ratio

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = open(os.path.join(ROOT, 'scflow_amd', 'csrc', 'corr_build_grad.hip')).read()
HEADER = open(os.path.join(ROOT, 'include', 'scflow_hip.h')).read()
U = 2.0 ** -24
CHUNK = 32                                      # CBG_KC: contraction steps staged at a time
TILE = 128                                      # CBG_TILE: channels / positions of a block

# (N, C, h, w): the smallest shapes at which each mechanism of the kernel can go wrong
SHAPES = [
    (1, 16, 4, 8),       # one fragment
    (3, 64, 8, 16),      # one tile, C below a tile, three samples
    (2, 256, 16, 16),    # exactly two tiles each way
    (1, 256, 12, 20),    # hw = 240: ragged tile and ragged 32-fragment, the chain test's map
    (2, 24, 5, 7),       # C % 16 != 0, hw % 4 != 0, sqrt(C) not a power of two: the division
    (1, 1, 1, 1),        # the smallest case
    (1, 256, 32, 32),    # the workload's map, eight tiles walked
]
EXACT_SHAPES = [s for s in SHAPES if s[1] in (16, 64, 256)]
assert {s[1] for s in EXACT_SHAPES} == {16, 64, 256}


# ============================================================================================================ float64
def c0(C):
    """roundings of the scale: 0 when sqrt(C) is a power of two (an exact product), else sqrtf's and the division's"""
    m, _ = np.frexp(np.sqrt(np.float32(C)))
    return 0 if m == 0.5 and float(np.sqrt(np.float32(C))) ** 2 == C else 2


def corr_build_grad64(g_vol, feat1, feat2, scale=None):
    """g_vol (N, hw, hw) or (N hw, h, w); feat1 / feat2 (N, C, h, w) -> (g_feat1, g_feat2) float64 (N, C, h, w)"""
    f1, f2 = f64(feat1), f64(feat2)
    n, c, h, w = f1.shape
    G = f64(g_vol).reshape(n, h * w, h * w)
    s = 1.0 / np.sqrt(float(c)) if scale is None else scale
    g1 = s * np.einsum('nij,ncj->nci', G, f2.reshape(n, c, h * w))
    g2 = s * np.einsum('nij,nci->ncj', G, f1.reshape(n, c, h * w))
    return g1.reshape(f1.shape), g2.reshape(f1.shape)


def corr_build_grad_ref(g_vol, feat1, feat2):
    """-> dict(g_feat1=(float64 value, bound), g_feat2=(...)): the bound of the module docstring, per element"""
    n, c, h, w = feat1.shape
    ref = corr_build_grad64(g_vol, feat1, feat2)
    mag = corr_build_grad64(np.abs(f64(g_vol)), np.abs(f64(feat1)), np.abs(f64(feat2)))
    k = h * w + c0(c)
    return dict(g_feat1=(ref[0], k * U * mag[0]), g_feat2=(ref[1], k * U * mag[1]))


def _rand(shape, seed):
    return torch.from_numpy(np.random.RandomState(seed).randn(*shape).astype(np.float32))


def grad_case(shape, seed=0):
    """random operands of a shape -> dict(g_vol (N hw, h, w), feat1, feat2), fp32 host tensors"""
    n, c, h, w = shape
    return dict(g_vol=_rand((n * h * w, h, w), 3 * seed + 11), feat1=_rand(shape, 3 * seed + 12), feat2=_rand(shape, 3 * seed + 13))


def exact_case(shape, seed=0):
    """small-integer operands: every product and partial sum is an integer below 2^24 and the scale a power of two, so
    the fp32 result IS the float64 one"""
    n, c, h, w = shape
    assert c0(c) == 0 and 16 * h * w < 2 ** 24
    rng = np.random.RandomState(100 + seed)
    ints = lambda s: torch.from_numpy(rng.randint(-4, 5, size=s).astype(np.float32))      # noqa: E731
    return dict(g_vol=ints((n * h * w, h, w)), feat1=ints(shape), feat2=ints(shape))


def worst(got, ref):
    """got: (g_feat1, g_feat2); ref: corr_build_grad_ref's -> worst error / bound over both outputs"""
    return max(worst_ratio(got[0], *ref['g_feat1']), worst_ratio(got[1], *ref['g_feat2']))


def torch_einsum32(g_vol, feat1, feat2):
    n, c, h, w = feat1.shape
    G = g_vol.reshape(n, h * w, h * w)
    sq = torch.sqrt(torch.tensor(float(c), dtype=torch.float32))
    g1 = torch.einsum('nij,ncj->nci', G, feat2.reshape(n, c, h * w)) / sq
    g2 = torch.einsum('nij,nci->ncj', G, feat1.reshape(n, c, h * w)) / sq
    return g1.reshape(feat1.shape), g2.reshape(feat1.shape)


def torch_autograd(g_vol, feat1, feat2, dtype=torch.float32):
    """autograd through level 0 of oracle.correlation_pyramid"""
    a, b = (t.detach().clone().to(dtype).requires_grad_() for t in (feat1, feat2))
    lvl0 = oracle.correlation_pyramid(a, b, 1)[0]
    (lvl0 * g_vol.to(dtype).reshape(lvl0.shape)).sum().backward()
    return a.grad, b.grad


# ============================================================================================================ defects
def _defect(name, case):
    """the two outputs a kernel with the planted defect would write (float64; an unwritten element keeps the 0 below)"""
    G, f1, f2 = f64(case['g_vol']), f64(case['feat1']), f64(case['feat2'])
    n, c, h, w = f1.shape
    hw = h * w
    G = G.reshape(n, hw, hw)
    good = corr_build_grad64(G, f1, f2)
    if name == 'outputs_swapped':
        return good[1], good[0]
    if name == 'volume_transposed':
        return corr_build_grad64(G.transpose(0, 2, 1), f1, f2)
    if name == 'scale_dropped':
        return corr_build_grad64(G, f1, f2, scale=1.0)
    if name == 'scale_twice':
        return corr_build_grad64(G, f1, f2, scale=1.0 / c)
    if name == 'last_ragged_chunk_dropped':       # the contraction stops at the last full chunk (at least one step dropped)
        keep = (hw - 1) // CHUNK * CHUNK
        Gj, Gi = G.copy(), G.copy()
        Gj[:, :, keep:] = 0
        Gi[:, keep:, :] = 0
        return corr_build_grad64(Gj, f1, f2)[0], corr_build_grad64(Gi, f1, f2)[1]
    if name == 'neighbour_sample':
        roll = lambda x: np.roll(x, 1, axis=0)     # noqa: E731
        return corr_build_grad64(G, f1, roll(f2))[0], corr_build_grad64(G, roll(f1), f2)[1]
    assert name in ('last_row_unwritten', 'last_column_unwritten'), name
    out = [g.copy() for g in good]
    for g in out:
        g = g.reshape(n, c, hw)
        if name == 'last_row_unwritten':
            g[:, min(c, TILE) - 1, :] = 0
        else:
            g[:, :, min(hw, TILE) - 1] = 0
    return tuple(out)


KERNEL_DEFECTS = ('outputs_swapped', 'volume_transposed', 'scale_dropped', 'scale_twice', 'last_ragged_chunk_dropped',
                  'neighbour_sample', 'last_row_unwritten', 'last_column_unwritten')


# ============================================================================================================ the tests
def test_symbol_is_declared_exported_bound_and_built():
    from scflow_amd import _lib, ops
    from scflow_amd.csrc import build
    from scflow_amd.modules import SCFlowDecoder
    from scflow_amd.refiner import SCFlowRefiner
    name = 'scf_corr_build_grad'
    assert f'int {name}(' in HEADER and f'extern "C" int {name}(' in SRC and name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES[name][1]) == 10 and hasattr(_lib.load(), name)
    assert 'corr_build_grad.hip' in build.SOURCES
    assert 'atomic' not in SRC.split('#include')[1]                 # no atomics: one summation order
    assert f'#define CBG_KC {CHUNK}' in SRC and f'#define CBG_TILE {TILE}' in SRC
    assert callable(ops.corr_build_grad) and callable(SCFlowDecoder.corr_backward)
    assert callable(SCFlowRefiner.loss_and_network_grads)


def test_c_abi_rejects_bad_arguments_before_any_launch():
    """every refusal returns before the stream is touched, so this runs without a GPU"""
    import ctypes as C
    from scflow_amd import _lib
    lib = _lib.load()
    bufs = [(C.c_float * 64)() for _ in range(5)]
    g, f1, f2, o1, o2 = (C.cast(b, C.c_void_p) for b in bufs)
    E, EUNSUP = -1, -2                          # scflow_hip.h: SCF_EINVAL, SCF_EUNSUPPORTED
    call = lambda g=g, f1=f1, f2=f2, o1=o1, o2=o2, N=1, C_=4, h=2, w=2: lib.scf_corr_build_grad(g, f1, f2, o1, o2, N, C_, h, w, None)  # noqa: E731
    for bad in (dict(g=None), dict(f1=None), dict(f2=None), dict(o1=None), dict(o2=None), dict(N=0), dict(N=-1), dict(C_=0),
                dict(h=0), dict(w=-2)):
        assert call(**bad) == E, bad
    # an output may alias neither the other output nor an input, not even in part
    part = C.cast(C.addressof(bufs[3]) + 4 * 15, C.c_void_p)            # the last float of o1's 16
    for bad in (dict(o2=o1), dict(o1=g), dict(o2=g), dict(o1=f1), dict(o1=f2), dict(o2=f1), dict(o2=f2), dict(o2=part)):
        assert call(**bad) == E, bad
    assert call(h=1 << 16, w=1 << 15) == EUNSUP
    # operands whose float counts would leave 63 bits as bytes are refused before they are multiplied out
    assert call(N=3, h=46340, w=46340) == EUNSUP and call(N=2 ** 31 - 1, C_=2 ** 30, h=1 << 15, w=1 << 15) == EUNSUP
    assert not any(any(b) for b in bufs)


@pytest.mark.parametrize('shape', SHAPES, ids=str)
def test_fp32_references_are_inside_the_bound(shape):
    """fp32 torch evaluations -- einsum, and autograd through oracle.correlation_pyramid's level 0 -- fall inside the
    bound at every shape; float64 autograd agrees with the restatement to float64 rounding"""
    case = grad_case(shape)
    ref = corr_build_grad_ref(**case)
    v = worst(torch_einsum32(**case), ref)
    measured(f'fp32 einsum {shape}: worst error / bound', v)
    assert v <= 1.0
    v = worst(torch_autograd(**case), ref)
    measured(f'fp32 autograd of the oracle\'s level 0 {shape}: worst error / bound', v)
    assert v <= 1.0
    a64 = torch_autograd(**case, dtype=torch.float64)
    for got, (want, _) in zip(a64, (ref['g_feat1'], ref['g_feat2'])):
        assert CH.rel(got.numpy(), want) <= 1e-13


@pytest.mark.parametrize('defect', KERNEL_DEFECTS)
def test_planted_defects_fall_outside_the_bound(defect):
    """every planted defect is outside the bound at every shape where it changes anything, by the margin printed"""
    margins = []
    for shape in SHAPES:
        n, c, h, w = shape
        if (defect == 'neighbour_sample' and n == 1) or (shape == (1, 1, 1, 1) and defect in (
                'outputs_swapped', 'volume_transposed', 'scale_dropped', 'scale_twice')):
            continue                              # the defect is the identity there
        case = grad_case(shape, seed=1)
        margins.append(worst(_defect(defect, case), corr_build_grad_ref(**case)))
    measured(f'planted {defect}: smallest worst error / bound over the shapes', min(margins))
    assert len(margins) >= 3 and min(margins) >= 100.0


@pytest.mark.parametrize('shape', EXACT_SHAPES, ids=str)
def test_small_integers_are_exact_in_fp32(shape):
    """the exactness operands the kernel test reuses: an fp32 evaluation has the float64 value's bits, in any order"""
    case = exact_case(shape)
    want = corr_build_grad64(**case)
    assert all(np.array_equal(w.astype(np.float32).astype(np.float64), w) for w in want)
    for got in (torch_einsum32(**case), torch_autograd(**case)):
        assert all(np.array_equal(f64(g), w) for g, w in zip(got, want))
    assert max(np.abs(w).max() for w in want) > 0


def test_doubling_the_cotangent_doubles_both_outputs():
    for shape in SHAPES:
        case = grad_case(shape, seed=2)
        a = torch_einsum32(**case)
        b = torch_einsum32(**dict(case, g_vol=case['g_vol'] * 2))
        assert all(torch.equal(x * 2, y) for x, y in zip(a, b)), shape


# ============================================================================================================ the join
import contextlib  # noqa: E402

import test_feature_grad_host as FH  # noqa: E402

GOLDEN = os.path.join(H.GOLDEN, 'network_grads.npz')
SMALL = dict(n=2, height=96, width=160, input_seed=3, case_seed=4)        # the chain test's small case: 12 x 20 maps
SMALL_ITERS, SMALL_FC1_IN = 2, 768
# ROOM[variant][group] of the two groups behind the volume, measured as tests/test_chain_grad_host.py measures its own: the
# reference's fp32 CPU autograd (network_grads.npz) against float64 at the fixture's inputs, max |g - g64| / max |g64|, as
# test_network_equals_the_reference_autograd printed it when the fixture was recorded.  'features': the two feature-map
# cotangents against the float64 chain's `correlation` carried through corr_build_grad64.  'render_encoder': the shared
# encoder's weights and head bias against float64 autograd of the encoder (FH.truth64) from that float64 cotangent;
# 'zero_bias': its biases in front of an InstanceNorm, |g| / sum |du| (exactly 0 in float64; FH.ZERO_BIAS_ROOM's measure).
ROOM = {
    'shipped': {'features': 0.000836, 'render_encoder': 0.00189, 'zero_bias': 5.04e-08},
    'raft': {'features': 0.000391, 'render_encoder': 0.00364, 'zero_bias': 4.15e-08},
}
# Why 'features' is three hundred times CH.ROOM's 'inputs', the group of the volume cotangent it is contracted from, and as
# large as CH.ROOM's 'encoder' (9.45e-4 / 1.2e-3), the group of the motion encoder that READS the volume: it has that
# group's cause.  The reference's fp32 forward differs from the float64 one in the last bits of every pose, hence by ~1e-4
# pixel in the re-projected flow the lookups are taken at, and the volume cotangent is taken at those other positions.
# Measured on the complete tensors (RAFT pose loss): feat_render 7.5e-4, feat_real 3.2e-4, and per sample 2e-6, 8e-4 / 3e-4
# and 3e-5 -- one sample of the three carries it, on both maps.  The stored pick (`feature_pick`, 1 / 512 of a map) happens
# to meet that sample's large entries on features.real (8.4e-4) and to miss them on features.render (2.5e-6): the two maps
# do not differ, the thinning does.  'inputs' does not see it because chain_grads.npz keeps every 768th query map only.
JOIN_DEFECTS = ('render_real_swapped', 'real_half_dropped', 'other_iteration_count', 'scale_missing')


def feature_pick(v):
    """the part of a feature-map cotangent (N, 256, h, w) network_grads.npz stores"""
    return v[:, ::32, ::4, ::4]


@contextlib.contextmanager
def feature_leaves():
    """inside: `chain_ref64` differentiates its ONE graph, in its own final torch.autograd.grad call, also at the two
    feature-map leaves the graph starts from -> dict, 'grads' = (d loss / d feat_render, d loss / d feat_real) after it.

    `chain_ref64` is imported, not edited, and returns no gradient at the feature maps; its graph is freed by its own
    grad call, so the only way to differentiate THAT graph there is inside that call.  This relies on two things about
    tests/test_chain_grad_host.py, both checked: it reaches the decoder through the name `oracle.scflow_decoder` with the
    two feature leaves first, and without a planted defect it calls `torch.autograd.grad` exactly once ('calls' counts
    them; `test_the_join_is_linear` asserts one decoder call and one grad call).  Both names are put back on the way out."""
    seen = {'calls': 0, 'decoder_calls': 0}
    decoder, grad = oracle.scflow_decoder, torch.autograd.grad

    def decoder_(feat_render, feat_real, *a, **k):
        seen['leaves'] = [feat_render, feat_real]
        seen['decoder_calls'] += 1
        return decoder(feat_render, feat_real, *a, **k)

    def grad_(total, targets, **kw):
        seen['calls'] += 1
        got = grad(total, list(targets) + seen['leaves'], **kw)
        seen['grads'] = tuple(g.detach().numpy() for g in got[-2:])
        return got[:-2]

    oracle.scflow_decoder, torch.autograd.grad = decoder_, grad_
    try:
        yield seen
    finally:
        oracle.scflow_decoder, torch.autograd.grad = decoder, grad


@lru_cache(maxsize=None)
def small_case():
    """the small case on the host -> (case, state dict, the decoder's four fp32 inputs from the CPU encoders)"""
    case = CH.chain_case(**SMALL)
    sd = CH.state_dict(0, fc1_in=SMALL_FC1_IN)
    with torch.no_grad():
        feats = oracle.extract_feat(case['inp']['render_images'], case['inp']['real_images'], sd)
    return case, sd, feats


def encoder_sd(sd, prefix='render_encoder.'):
    return {k[len(prefix):]: v for k, v in sd.items() if k.startswith(prefix)}


def join64(res, feats):
    """a chain result and the decoder inputs it started from -> the float64 (d loss / d feat_render, d loss / d feat_real)"""
    return corr_build_grad64(res['correlation'], feats[0], feats[1])


@lru_cache(maxsize=None)
def _fixture_encoder():
    """the float64 forward of the shared encoder on the fixture's 2N stacked images (render first), once"""
    case = CH.fixture_case('shipped')[0]
    esd = encoder_sd(CH.state_dict(CH.FIXTURE_SEEDS['weight_seed']))
    x = torch.cat([case['inp']['render_images'], case['inp']['real_images']])
    with torch.no_grad():
        acts = FH.forward64(x, esd)
    return x, esd, acts


def encoder_truth64(images, sd, g_features, relu=None, ties=None):
    """float64 autograd of the shared feature encoder on the 2N stacked images (render first) from the stacked float64
    cotangent -> (the 32 gradients as arrays, FH.zero_bias_scales of the same walk)"""
    x = torch.cat([t.detach().cpu() for t in images])
    g = torch.from_numpy(np.concatenate(g_features))
    esd = encoder_sd(sd)
    acts, truth = FH.truth64(x, esd, g, relu=relu, ties=ties)
    launches = {}
    FH.backward_ref64(acts, esd, g, launches=launches)
    return {k: v.numpy() for k, v in truth.items()}, FH.zero_bias_scales(launches)


@lru_cache(maxsize=None)
def fixture_truth(variant, defect=None):
    """float64 at the fixture's inputs -> (features (render, real), encoder gradients, zero-bias scales).  The undamaged
    encoder gradients are float64 autograd (`encoder_truth64`).  ``defect``: one of JOIN_DEFECTS planted into the join; its
    encoder gradients come from FH.backward_ref64, the float64 walk that tests/test_feature_grad_host.py holds to autograd
    within 1e-11, on the one cached forward.  Shared: do not write."""
    case, res = CH.fixture_case(variant)
    feats = CH.fixture_decoder_inputs()
    sd = CH.state_dict(CH.FIXTURE_SEEDS['weight_seed'])
    if defect is None:
        g = join64(res, feats)
        return (g,) + encoder_truth64((case['inp']['render_images'], case['inp']['real_images']), sd, g)
    g = features = join64(res, feats)
    if defect == 'render_real_swapped':           # the two maps handed to the stage in the other order
        g = features = corr_build_grad64(res['correlation'], feats[1], feats[0])
    elif defect == 'scale_missing':
        g = features = corr_build_grad64(res['correlation'], feats[0], feats[1], scale=1.0)
    elif defect == 'other_iteration_count':       # the volume cotangent of a chain one iteration shorter
        short = CH.chain_ref64(feats, CH.decoder_sd64(sd), CH.chain_data(case), CH.chain_cfgs(case, variant), CH.shipped_flags(),
                               iters=H.REFINER_ITERS - 1, variant=variant)
        g = features = join64(short, feats)
    else:                                         # the shared encoder's sum without the real images' half
        assert defect == 'real_half_dropped', defect
        g = (g[0], np.zeros_like(g[1]))
    _, esd, acts = _fixture_encoder()
    launches = {}
    params = FH.backward_ref64(acts, esd, torch.from_numpy(np.concatenate(g)), launches=launches)
    return features, params, FH.zero_bias_scales(launches)


def network_flat(features, params):
    """-> {compared key: array}: 'features.render', 'features.real' and the 32 'render_encoder.*'"""
    out = {'features.render': f64(features[0]), 'features.real': f64(features[1])}
    out.update(('render_encoder.' + k, f64(params[k])) for k in FH.PARAM_NAMES)
    return out


def network_measures(got, truth, scales, pick=False):
    """`network_flat` dicts (``got`` already thinned when ``pick``) -> {group: the measure of its ROOM}"""
    worst = dict(features=0.0, render_encoder=0.0, zero_bias=0.0)
    for k, want in truth.items():
        name = k.split('.', 1)[1]
        if k.startswith('features.'):
            worst['features'] = max(worst['features'], CH.rel(got[k], feature_pick(want) if pick else want))
        elif name in FH.ZERO_BIASES:
            assert np.abs(want).max() <= 1e-9 * scales[name].max(), k           # float64: zero up to its own rounding
            worst['zero_bias'] = max(worst['zero_bias'], float((np.abs(got[k]) / scales[name]).max()))
        else:
            have, top = got[k], np.abs(want).max()
            want = FH.golden_pick(name, want) if pick else want
            assert have.shape == want.shape and top > 0, k
            worst['render_encoder'] = max(worst['render_encoder'], float(np.abs(have - want).max() / top))
    return worst


@pytest.mark.parametrize('variant', CH.VARIANTS)
def test_the_join_is_linear(variant):
    """`chain_ref64`'s `correlation` carried through `corr_build_grad64` IS the gradient of the same float64 graph at the
    two feature maps it starts from (one autograd call, `feature_leaves`): to 1e-12 of the largest entry"""
    case, sd, feats = small_case()
    with feature_leaves() as seen:
        res = CH.chain_ref64(feats, CH.decoder_sd64(sd), CH.chain_data(case), CH.chain_cfgs(case, variant), CH.shipped_flags(),
                             iters=SMALL_ITERS, variant=variant)
    assert seen['calls'] == 1 and seen['decoder_calls'] == 1, 'chain_ref64 no longer makes one decoder and one grad call'
    assert res['correlation'].shape == (2 * 240, 12, 20) and np.abs(res['correlation']).max() > 0
    for name, got, want in zip(('render', 'real'), join64(res, feats), seen['grads']):
        v = CH.rel(got, want)
        measured(f'{variant}: corr_build_grad64 of the chain\'s volume cotangent vs one-graph autograd, feat_{name}', v)
        assert v <= 1e-12 and np.abs(want).max() > 0
    # the hook is gone: a plain chain run leaves the patched names as they were
    assert oracle.scflow_decoder.__name__ == 'scflow_decoder' and torch.autograd.grad.__module__ == 'torch.autograd'


@pytest.mark.parametrize('variant', CH.VARIANTS)
def test_network_equals_the_reference_autograd(variant):
    """the reference's own fp32 CPU backward through the whole network (network_grads.npz) against float64 at the
    fixture's inputs: where ROOM of the two groups behind the volume is measured, and held to 1.5 x what is recorded"""
    z = np.load(GOLDEN)
    assert {k: int(z[k]) for k in CH.FIXTURE_SEEDS} == CH.FIXTURE_SEEDS and int(z['iters']) == H.REFINER_ITERS
    assert os.path.getsize(GOLDEN) < 200 * 1024
    assert all(z[k].dtype in (np.float32, np.int32, np.int64) or z[k].dtype.kind == 'U' for k in z.files)
    features, params, scales = fixture_truth(variant)
    truth = network_flat(features, params)
    assert sorted(f'{variant}.{k}' for k in truth) == sorted(k for k in z.files if k.startswith(variant + '.') and
                                                            k != f'{variant}.loss')
    assert abs(float(z[f'{variant}.loss']) - CH.fixture_case(variant)[1]['loss']) <= 1e-4 * abs(float(z[f'{variant}.loss']))
    got = {k: f64(z[f'{variant}.{k}']) for k in truth}
    worst = network_measures(got, truth, scales, pick=True)
    for group, v in sorted(worst.items()):
        measured(f'reference fp32 autograd vs float64, {variant}, {group}', v)
    for group, v in sorted(worst.items()):
        assert v <= 1.5 * ROOM[variant][group], (group, v)
    assert sorted(worst) == sorted(ROOM[variant])


@pytest.mark.parametrize('defect', JOIN_DEFECTS)
def test_planted_join_defects_leave_the_room(defect):
    """every join defect moves a compared tensor at least 10 rooms away from the undamaged float64 values: the GPU tests'
    2 x ROOM would see it five times over.  A condition on the inputs (FIXTURE_SEEDS)."""
    for variant in CH.VARIANTS:
        good_f, good_p, scales = fixture_truth(variant)
        bad_f, bad_p, _ = fixture_truth(variant, defect)
        good, bad = network_flat(good_f, good_p), network_flat(bad_f, bad_p)
        ratios = {}
        for k in good:
            name = k.split('.', 1)[1]
            if name in FH.ZERO_BIASES:
                continue
            group = 'features' if k.startswith('features.') else 'render_encoder'
            ratios[k] = CH.rel(bad[k], good[k]) / ROOM[variant][group]
        k = max(ratios, key=ratios.get)
        measured(f'planted {defect}, {variant}: largest deviation / room ({k})', ratios[k])
        assert ratios[k] >= 10.0, (variant, k, ratios[k])
