"""randomised sweep of scf_conv2d_pair (ops.conv2d_pair): two independent convolutions, merged into one launch where the rule table
pairs their families, checked per case against
  - two separate ops.conv2d calls and the same pair with tune('conv_pair', 1): bit for bit;
  - a CPU float64 restatement (conv, bias, BN, residual, activation in double): 40 eps * sum|w||x| (the conv_fuzz bound), plus the
    3e-7 of the hardware tanh / sigmoid forms (scf_common.h) for those epilogues;
  - guard bands: outputs are channel slices of NaN-filled buffers, nothing outside a slice is written, everything inside is finite;
  - the dispatch log: each layer under the family its single launch takes, paired = [0, 0] or [1, 2].
The draw picks a target first, one pair-kernel instantiation or a pair that does not merge (merging needs small grids: batch 1-4,
maps of 8..64, or two Winograd grids of half a round each), then per layer the batch and map size, bias / BN / residual, act / act_split + act2, a channel-slice input view, an ``out=`` channel slice and two input segments.
``stats`` (a dict) collects the merged family pairs and pair-kernel instantiations that ran.
    python tools/lab/pair_fuzz.py [cases] [seed]"""
import collections
import os
import random
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch
import torch.nn.functional as F
from scflow_amd import ops
DEV = 'cuda:0'
EPS = 1.19e-7
ACTS = (ops.ACT_NONE, ops.ACT_RELU, ops.ACT_TANH, ops.ACT_SIGMOID)
ACT_NAMES = {ops.ACT_NONE: 'none', ops.ACT_RELU: 'relu', ops.ACT_TANH: 'tanh', ops.ACT_SIGMOID: 'sigmoid'}
FLOP_CAP = 1e9          # per layer: the fp64 reference of a case stays under ~2e9 flops
# what a case aims at: every pair-kernel instantiation (the merged family pair follows from it), pairs of pairable families past
# one round of resident blocks, and families the rule table does not pair.  Each seed draws every target equally often.
_X = ('dword', 'x4')
TARGETS = tuple(f'dma_pair<{s}, NG{g}>' for s in _X for g in (1, 2)) + tuple(f'dma_taps_pair<{s}, NG{g}>' for s in _X for g in (1, 2)) + \
    tuple(f'taps_pair<{a}, {b}>' for a in (32, 64) for b in (32, 64)) + ('thin_pair<324, 110>',) + \
    tuple(f'wino_q_pair<{s}>' for s in _X) + tuple(f'wino_mixed_pair<{q}, {p}>' for q in _X for p in _X) + ('no-pay', 'no-rule')


def _geom(rs, k, hw, n, cin, cout, stride=1, pad=None):
    return dict(k=k, pad=pad if pad is not None else (k[0] // 2, k[1] // 2), stride=stride, hw=hw, n=n, cin=cin, cout=cout)


def _width(rs, x4, lo, hi, even=False):
    """a map width in [lo, hi]: W % 4 == 0 (rows keep 16-byte alignment: the x4 patch staging) or not"""
    while True:
        w = rs.randint(lo, hi)
        if (w % 4 == 0) == x4 and (not even or w % 2 == 0):
            return w


def _dma(rs, x4, tiny):
    """a layer for the K-split LDS-DMA tile.  ``tiny``: a 1x1 layer of >= 4 channel chunks on a grid of at most one block per CU
    (two wave groups per block, NG = 2); else a small grid of any kind"""
    if tiny:
        h = rs.randint(8, 16)
        return _geom(rs, (1, 1), (h, _width(rs, x4, 8, 16)), 1, rs.choice([128, 192, 256]), rs.choice([32, 64, 128]))
    kind = rs.choice(['3x3', '3x3', '1x1', '1x1'] + ([] if x4 else ['1x1/s2', '3x3/s2']))
    # mostly one or two channel chunks: a block keeps one wave group (NG = 1) whatever the grid
    cin = rs.choice([16, 24, 32]) if rs.random() < 0.6 else rs.choice([64, 96, 128, 192, 256] + ([] if kind.startswith('3x3') else [324]))
    cout = rs.choice([32, 64, 96, 128, 192, 256])
    h = rs.choice([16, 24, 32]) if rs.random() < 0.5 else rs.randint(6, 32)
    hw, n = (h, _width(rs, x4, 16 if kind.startswith('3x3') else 6, 32)), rs.choice([1, 1, 1, 2])
    if kind == '3x3':
        return _geom(rs, (3, 3), hw, n, cin, min(cout, 192) if cin > 192 else cout)
    if kind == '3x3/s2':
        return _geom(rs, (3, 3), hw, n, cin, cout, stride=2)
    if kind == '1x1/s2':
        return _geom(rs, (1, 1), hw, n, cin, cout, stride=2, pad=(0, 0))
    return _geom(rs, (1, 1), hw, n, cin, cout)


def _taps(rs, wide=False):
    """a layer for the thin-input kernel (Cin <= 4).  ``wide``: batch 32 at 32 x 32 with 128 output channels, the grid on which a
    block takes 64 output channels; else 32 per block (small grids, or the encoder stems at 256 x 256)"""
    k = rs.choice([(7, 7), (3, 3), (5, 5), (3, 3)])
    if wide:
        return _geom(rs, k, rs.choice([(32, 32), (30, 32), (32, 29)]), 32, rs.choice([1, 2]), 128)
    if rs.random() < 0.15:
        return _geom(rs, (7, 7), rs.choice([(256, 256), (240, 256)]), rs.choice([1, 2]), 3, 64, stride=2)
    hw = rs.choice([(32, 32), (30, 30), (32, 28)]) if rs.random() < 0.5 else (rs.randint(8, 40), rs.randint(8, 40))
    return _geom(rs, k, hw, rs.choice([1, 1, 2, 3]), rs.choice([1, 2, 3, 4]), rs.choice([32, 64, 64, 128]))


def _thin(rs, first):
    """flow prediction (3x3 -> 2, one block row per CU) | mask prediction (1x1 -> 1)"""
    cin = rs.choice([32, 64, 128, 256])
    n = rs.choice([1, 1, 2, 4])
    hw = rs.choice([(32, 32), (32, 20)]) if rs.random() < 0.5 else (rs.randint(6, 32), rs.randint(6, 32))
    return _geom(rs, (3, 3), hw, n, cin, 2) if first else _geom(rs, (1, 1), hw, n, cin, 1)


def _wino_blocks(n, ho, wo, cout, quarter):
    """blocks of a F(2x2, 3x3) launch (the tile-group geometry of scf_conv_wino_dispatch), only to size the draw"""
    tcols, txl = (wo + 1) // 2, 4
    best = (tcols + 15) // 16 * 16
    if tcols < 16:
        txl, best = max(2, (tcols - 1).bit_length()), 0
    for l in (3, 2):
        if not best:
            break
        wpad = (tcols + (1 << l) - 1) >> l << l
        if wpad * 10 <= best * 9:
            best, txl = wpad, l
    txw, tyw, f = 1 << txl, 32 >> txl, (cout + 31) // 32
    tw = 1 if quarter else 2
    return n * -(-wo // (2 * txw)) * -(-ho // (2 * tw * tyw)) * (f // 2 if quarter else f)


def _wino(rs, quarter, x4):
    """a 3x3 / stride-1 layer of 128..256 Winograd blocks (>= CUs / 2, and two such grids fit the chip together): an even fragment
    count takes the quarter-domain kernel, an odd one the pair kernel"""
    cout = rs.choice([64, 128]) if quarter else rs.choice([32, 96])
    h, w = rs.randint(40, 64), (rs.choice([64, 80]) if x4 else rs.choice([54, 62, 66, 70, 74, 78])) if quarter else \
        _width(rs, x4, 40, 80, even=True)
    n = max(1, min(16, 192 // max(1, _wino_blocks(1, h, w, cout, quarter))))
    return _geom(rs, (3, 3), (h, w), n, rs.choice([8, 16, 32] if quarter else [8, 16]), cout)


def draw_pair(rs, t):
    """-> (geometry a, geometry b) of a case aimed at target ``t``"""
    x4 = lambda name: '<x4' in name or ', x4' in name
    if t.startswith('dma_pair'):
        tiny = t.endswith('NG2>')
        return _dma(rs, x4(t), tiny), _dma(rs, x4(t), tiny)
    if t.startswith('dma_taps_pair'):
        a, b = _dma(rs, x4(t), t.endswith('NG2>')), _taps(rs)
        return (a, b) if rs.random() < 0.5 else (b, a)
    if t.startswith('taps_pair'):
        return _taps(rs, wide=t[10:12] == '64'), _taps(rs, wide=t[14:16] == '64')
    if t.startswith('thin_pair'):
        return _thin(rs, True), _thin(rs, False)
    if t.startswith('wino_q_pair'):
        return _wino(rs, True, x4(t)), _wino(rs, True, x4(t))
    if t.startswith('wino_mixed_pair'):
        q, p = t[16:-1].split(', ')
        a, b = _wino(rs, True, q == 'x4'), _wino(rs, False, p == 'x4')
        return (a, b) if rs.random() < 0.5 else (b, a)
    if t == 'no-pay':             # pairable families on grids past one round of resident blocks
        return (_geom(rs, (3, 3), (32, 32), 2, 128, rs.choice([128, 192])),
                _geom(rs, (3, 3), (32, 32), 2, rs.choice([64, 128]), rs.choice([64, 128])))
    r = rs.random()               # families the rule table does not pair: K-split | thin-output, F(4, 5), the register-staged kernel
    if r < 0.4:
        return _dma(rs, rs.random() < 0.5, False), _thin(rs, True)
    if r < 0.7:
        return _geom(rs, rs.choice([(1, 5), (5, 1)]), rs.choice([(60, 80), (64, 64), (48, 60)]), rs.choice([2, 4]),
                     rs.choice([16, 32, 64]), 64), _dma(rs, rs.random() < 0.5, False)
    return _geom(rs, (5, 5), (rs.randint(8, 40), rs.randint(8, 40)), rs.choice([1, 2]), rs.choice([5, 6, 7]),
                 rs.choice([8, 20, 40])), _taps(rs)


def _epilogue(rs, g, strict):
    """per-layer draws; ``strict``: keep to what the target family takes (thin-output: no BN / residual / split / segments; Winograd:
    ReLU-or-none, no split; thin-input: one segment), so that most draws still land on the target"""
    fam_thin, fam_wino, fam_taps = g['cout'] <= 4, g['k'] == (3, 3) and g['stride'] == 1 and g['hw'][0] >= 40, g['cin'] <= 4
    e = dict(bias=rs.random() < 0.8, bn=rs.random() < 0.25, res=rs.random() < 0.25, act=rs.choice(ACTS), act2=ops.ACT_NONE, split=0,
             c0=0, in_view=None, out_view=None)
    if g['cout'] > 1 and rs.random() < 0.3:
        e['act2'] = rs.choice(ACTS)
        on32 = [c for c in range(32, g['cout'], 32)]
        e['split'] = rs.choice(on32) if on32 and rs.random() < 0.5 else rs.randint(1, g['cout'] - 1)
    if g['cin'] >= 16 and rs.random() < 0.25:
        on = [c for c in (32, 64, 96, 128, 192) if c < g['cin']]
        e['c0'] = rs.choice(on) if on and rs.random() < 0.5 else rs.choice([c for c in range(1, g['cin']) if c % 8])
    if rs.random() < 0.4:           # input = channels [lo, lo + Cin) of a wider tensor: sample stride and 16-byte alignment move
        e['in_view'] = (rs.randint(0, 5), rs.randint(0, 5))
    if rs.random() < 0.6:           # out = channels [lo, lo + Cout) of a wider buffer
        e['out_view'] = (rs.randint(0, 40), rs.randint(0, 40))
    if strict:
        if fam_thin:
            e.update(bn=False, res=False, split=0, c0=0)
        if fam_wino:
            e.update(split=0)
            if e['act'] not in (ops.ACT_NONE, ops.ACT_RELU):
                e['act'] = rs.choice([ops.ACT_NONE, ops.ACT_RELU])
        if fam_taps:
            e['c0'] = 0
    return e


class _Layer:
    def __init__(self, g, e, gen):
        self.g, self.e = g, e
        n, cin, cout, (kh, kw), (ph, pw), s = g['n'], g['cin'], g['cout'], g['k'], g['pad'], g['stride']
        H, W = g['hw']
        self.ho, self.wo = (H + 2 * ph - kh) // s + 1, (W + 2 * pw - kw) // s + 1
        lo, hi = e['in_view'] or (0, 0)
        self.xw = torch.randn((n, lo + cin + hi, H, W), generator=gen)
        self.x = self.xw[:, lo:lo + cin]
        self.w = torch.randn((cout, cin, kh, kw), generator=gen) * (1.0 / (cin * kh * kw)) ** 0.5
        self.b = torch.randn((cout,), generator=gen) * 0.1 if e['bias'] else None
        self.bn = None
        if e['bn']:
            self.bn = (torch.randn((cout,), generator=gen) * 0.2 + 1, torch.randn((cout,), generator=gen) * 0.1,
                       torch.randn((cout,), generator=gen) * 0.1, torch.rand((cout,), generator=gen) * 0.5 + 0.5)
        self.r = torch.randn((n, cout, self.ho, self.wo), generator=gen) if e['res'] else None

    def flops(self):
        g = self.g
        return 2.0 * g['n'] * g['cin'] * g['k'][0] * g['k'][1] * g['cout'] * self.ho * self.wo

    def to_device(self):
        g, e = self.g, self.e
        self.pc = ops.PackedConv.from_weight(self.w.to(DEV), None if self.b is None else self.b.to(DEV), stride=g['stride'],
                                             padding=g['pad'], bn=None if self.bn is None else [t.to(DEV) for t in self.bn])
        lo = (e['in_view'] or (0, 0))[0]
        xw = self.xw.to(DEV)
        x = xw[:, lo:lo + g['cin']]
        self.x0, self.x1 = (x[:, :e['c0']], x[:, e['c0']:]) if e['c0'] else (x, None)
        self.rd = None if self.r is None else self.r.to(DEV)

    def out(self):
        """-> (wide NaN buffer or None, the view the layer writes or None)"""
        if self.e['out_view'] is None:
            return None, None
        lo, hi = self.e['out_view']
        wide = torch.full((self.g['n'], lo + self.g['cout'] + hi, self.ho, self.wo), float('nan'), device=DEV)
        return wide, wide[:, lo:lo + self.g['cout']]

    def kwargs(self, out):
        e = self.e
        return dict(x1=self.x1, out=out, res=self.rd, act=e['act'], act2=e['act2'], act_split=e['split'])

    def want(self):
        g, e = self.g, self.e
        y = F.conv2d(self.x.double(), self.w.double(), None if self.b is None else self.b.double(), stride=g['stride'], padding=g['pad'])
        if self.bn is not None:
            ga, be, mu, var = (t.double()[None, :, None, None] for t in self.bn)
            y = (y - mu) / torch.sqrt(var + 1e-5) * ga + be
        if self.r is not None:
            y = y + self.r.double()
        acts = [e['act']] * g['cout']
        if e['split'] > 0:
            acts[e['split']:] = [e['act2']] * (g['cout'] - e['split'])
        fn = {ops.ACT_NONE: lambda v: v, ops.ACT_RELU: torch.relu, ops.ACT_TANH: torch.tanh, ops.ACT_SIGMOID: torch.sigmoid}
        return torch.cat([fn[a](y[:, c:c + 1]) for c, a in enumerate(acts)], 1) if len(set(acts)) > 1 else fn[acts[0]](y)

    def limit(self):
        """40 eps * sum |w||x| per output (conv_fuzz's estimate: mean |x| times the largest row sum of |w|), scaled by the folded BN
        scale; + 3e-7 when a tanh / sigmoid runs in the epilogue"""
        e = self.e
        s = float(self.x.abs().double().mean() * self.w.abs().double().sum(dim=(1, 2, 3)).max())
        if self.bn is not None:
            s *= max(1.0, float((self.bn[0] / torch.sqrt(self.bn[3] + 1e-5)).abs().max()))
        trans = {e['act'], e['act2'] if e['split'] > 0 else ops.ACT_NONE} & {ops.ACT_TANH, ops.ACT_SIGMOID}
        return 40 * EPS * max(s, 1.0) + 1e-6 + (3e-7 if trans else 0.0)

    def tag(self):
        g, e = self.g, self.e
        v = '' if e['in_view'] is None else f' in[{e["in_view"][0]}:+{g["cin"]}:+{e["in_view"][1]}]'
        o = '' if e['out_view'] is None else f' out[{e["out_view"][0]}:+{g["cout"]}:+{e["out_view"][1]}]'
        sp = f' split{e["split"]}->{ACT_NAMES[e["act2"]]}' if e['split'] else ''
        return (f'N{g["n"]} {g["cin"]}->{g["cout"]} {g["k"][0]}x{g["k"][1]}/s{g["stride"]} @{g["hw"][0]}x{g["hw"][1]} c0={e["c0"]} '
                f'bias={int(e["bias"])} bn={int(e["bn"])} res={int(e["res"])} {ACT_NAMES[e["act"]]}{sp}{v}{o}')


def instantiation(fa, fb, va, vb):
    """the pair-kernel instantiation a merged launch of families fa | fb with captured variants va | vb ran"""
    px4 = lambda v: 'x4' if v & 1 else 'dword'
    if fa == fb == 'direct-dma':
        return f'dma_pair<{px4(va)}, NG{1 + (va >> 1)}>'
    if {fa, fb} == {'direct-dma', 'taps'}:
        v = va if fa == 'direct-dma' else vb
        return f'dma_taps_pair<{px4(v)}, NG{1 + (v >> 1)}>'
    if fa == fb == 'taps':
        return f'taps_pair<{32 * va}, {32 * vb}>'
    if fa == fb == 'thin':
        return f'thin_pair<{va}, {vb}>'
    if fa == fb == 'winograd-q':
        return f'wino_q_pair<{px4(va - 10)}>'
    if {fa, fb} == {'winograd-q', 'winograd'}:
        q, p = (va, vb) if fa == 'winograd-q' else (vb, va)
        return f'wino_mixed_pair<{px4(q - 10)}, {px4(p - 20)}>'
    return f'{fa}|{fb}?'


def _pair(la, lb, outs):
    return ops.conv2d_pair((la.pc, la.x0, la.kwargs(outs[0])), (lb.pc, lb.x0, lb.kwargs(outs[1])))


def run(cases: int, seed: int, verbose: bool = True, stats: dict = None) -> int:
    """-> number of failing cases"""
    _print = print if verbose else (lambda *a, **k: None)
    rs = random.Random(seed)
    torch.set_num_threads(16)
    st = stats if stats is not None else {}
    for key in ('targets', 'families', 'merged', 'instantiations'):
        st.setdefault(key, collections.Counter())
    st.setdefault('worst', 0.0)
    bad = 0
    order = []
    for ci in range(cases):
        if not order:
            order = list(TARGETS)
            rs.shuffle(order)
        target = order.pop()
        ga, gb = draw_pair(rs, target)
        strict = rs.random() < 0.9
        ea, eb = _epilogue(rs, ga, strict), _epilogue(rs, gb, strict)
        gen = torch.Generator().manual_seed(seed * 100003 + ci)
        la, lb = _Layer(ga, ea, gen), _Layer(gb, eb, gen)
        for lay in (la, lb):            # fp64 reference budget: fewer samples, never an empty output
            while lay.flops() > FLOP_CAP and lay.g['n'] > 1:
                lay.g['n'] = max(1, lay.g['n'] // 2)
                lay.__init__(lay.g, lay.e, gen)
        tag = f'case {ci} [{target}]: a = {la.tag()} | b = {lb.tag()}'
        try:
            la.to_device()
            lb.to_device()
            (wa1, va1), (wb1, vb1) = la.out(), lb.out()
            with ops.record_conv_kernels() as single:
                want_a = ops.conv2d(la.pc, la.x0, **la.kwargs(va1))
                want_b = ops.conv2d(lb.pc, lb.x0, **lb.kwargs(vb1))
            (wa, va), (wb, vb) = la.out(), lb.out()
            rec = ops.record_conv_kernels()
            with rec as ran:
                got_a, got_b = _pair(la, lb, (va, vb))
            (wa2, va2), (wb2, vb2) = la.out(), lb.out()
            prev = ops.tune('conv_pair', 1)
            try:
                rec2 = ops.record_conv_kernels()
                with rec2:
                    two_a, two_b = _pair(la, lb, (va2, vb2))
            finally:
                ops.tune('conv_pair', prev)
            torch.cuda.synchronize()
        except Exception as exc:
            print('RAISED', tag, repr(exc)[:300], flush=True)
            bad += 1
            continue
        why = []
        fams = [f for _, f in single]
        fa, fb = (fams + ['?', '?'])[:2]
        pair_name = f'{fa}|{fb}'
        st['targets'][target] += 1
        st['families'][pair_name] += 1
        if len(ran) != 2 or ran != single:
            why.append(f'log {ran} != single launches {single}')
        if rec.paired not in ([0, 0], [1, 2]) or rec2.paired != [0, 0]:
            why.append(f'paired {rec.paired} / {rec2.paired}')
        merged = rec.paired == [1, 2]
        if merged:
            st['merged'][pair_name] += 1
            st['instantiations'][instantiation(fa, fb, *rec.variants)] += 1
        if not (torch.equal(got_a, want_a) and torch.equal(got_b, want_b)):
            why.append('pair != two conv2d calls')
        if not (torch.equal(two_a, want_a) and torch.equal(two_b, want_b)):
            why.append("tune('conv_pair', 1) != two conv2d calls")
        errs = []
        for name, lay, got, wide in (('a', la, got_a, wa), ('b', lb, got_b, wb)):
            if not bool(torch.isfinite(got).all()):
                why.append(f'{name}: non-finite output')
            if wide is not None:
                lo = lay.e['out_view'][0]
                outside = torch.ones(wide.shape[1], dtype=torch.bool)
                outside[lo:lo + lay.g['cout']] = False
                if not bool(torch.isnan(wide[:, outside.to(DEV)]).all()):
                    why.append(f'{name}: wrote outside its output slice')
            err = float((got.cpu().double() - lay.want()).abs().max())
            lim = lay.limit()
            st['worst'] = max(st['worst'], err / lim)
            errs.append(f'{err:.2e}/{lim:.2e}')
            if not err <= lim:
                why.append(f'{name}: err {err:.2e} > {lim:.2e}')
        if why:
            bad += 1
            print('FAIL', tag, f'[{pair_name} paired {rec.paired} variants {rec.variants}]', '; '.join(why), flush=True)
        else:
            _print(f'ok   {tag} [{pair_name}{" merged " + instantiation(fa, fb, *rec.variants) if merged else ""}] err {" ".join(errs)}',
                   flush=True)
    _print('families:', dict(st['families']))
    _print('merged:', dict(st['merged']))
    _print('instantiations:', dict(st['instantiations']))
    _print(f'worst err / bound: {st["worst"]:.3f}')
    print('FUZZ', 'FAILED' if bad else 'ok', bad, 'of', cases, flush=True)
    return bad


if __name__ == '__main__':
    sys.exit(1 if run(int(sys.argv[1]) if len(sys.argv) > 1 else 300, int(sys.argv[2]) if len(sys.argv) > 2 else 0) else 0)
