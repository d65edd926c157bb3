"""The six optimizer steps beside Adam and the Philox draws of csrc/tdg_elementwise.hip against the float64 references of
tests/_exact_steps.py, per element and per output array: bit for bit where the recipe makes exactness provable (the
accumulators at power-of-two decays, all of the momentum step, the uniform draw, the _dev forms against the host-offset
forms), against derived bounds where it cannot be.  g is NaN-guarded and must keep its bits, p, every slot and every
draw are sentinel-guarded, one case of each puts the base off the buffer's start.  The conditions of the exact
comparisons are proved for the whole case table on the CPU (tests/test_host_steps_exact.py); nothing here skips.

Each bounded comparison prints its worst ratio (`RATIO <what> <value>`, run with -s); DESIGN.md section 2 records them."""
import numpy as np
import pytest
import torch

from conftest import pkg
import _exact_pointwise as P
import _exact_steps as S

pytestmark = pytest.mark.gpu

ES = {0: 4, 1: 2}
DT = {0: 'f32', 1: 'bf16'}
TAIL = 16


def K():
    return pkg('kernels')


def call(name, *args):
    pkg('_lib').call(name, *args)


def refused(name, *args):
    """TDG_EINVAL with the entry's own name in front of tdg_last_error()."""
    lib = pkg('_lib').load()
    assert getattr(lib, name)(*args) == -1, name
    msg = lib.tdg_last_error().decode()
    assert msg.startswith(name + ':'), msg
    return msg


def dev():
    return torch.device('cuda:0')


def exact(got, want, what):
    assert np.array_equal(got, want), '%s\n%s' % (what, P.describe_mismatch(np.asarray(got), np.asarray(want)))


def within(ratio, what):
    """`ratio`: |error| / bound per element (inf: an exact output whose bits differ).  Prints the worst one, then asserts it."""
    worst = float(np.max(ratio)) if np.size(ratio) else 0.0
    print('RATIO %s %.4g' % (what, worst))
    if not worst <= 1.0:
        bad = np.argwhere(~(np.asarray(ratio) <= 1.0))
        raise AssertionError('%s: %d of %d miss the bound, worst ratio %g, first at %s'
                             % (what, len(bad), np.size(ratio), worst, tuple(int(i) for i in bad[0])))


class Vec:
    """n live elements on the device with `off` guard elements in front and TAIL behind.  data=None: an output, all sentinel.
    The guards hold `fill`: NaN for an input that is only read, the sentinel for whatever the kernel writes."""

    def __init__(self, n, off=0, data=None, fill=P.SENTINEL, dtype=0):
        self.n, self.off, self.fill, self.dtype = n, off, fill, dtype
        flat = np.full(off + n + TAIL, fill if data is not None else P.SENTINEL, dtype=np.float32)
        if data is not None:
            flat[off:off + n] = data
        self.t = torch.from_numpy(flat).to(dev()).to(K().TORCH_DTYPE[dtype])

    def ptr(self):
        return K().ptr(self.t, self.off * ES[self.dtype])

    def guards_intact(self):
        g = torch.cat([self.t[:self.off], self.t[self.off + self.n:]]).float().cpu().numpy()
        ok = np.isnan(g) if np.isnan(self.fill) else g == self.fill
        assert np.all(ok), '%d guard elements were overwritten' % int((~ok).sum())

    def get(self):
        """The live values, after asserting that nothing outside them has changed."""
        self.guards_intact()
        return self.t[self.off:self.off + self.n].float().cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ------------------------------------------------------------------------------------------------ 1. optimizer steps
def run_step(name, cfg, n, off, n_launches=2, period=S.TABLE):
    st, h = S.STEPS[name], S.hyper(name, cfg)
    table = S.step_inputs(name, cfg)
    inp = S.prefix(table, n, period)
    bufs = {a: Vec(n, off, inp[a], fill=P.NAN if a == 'g' else P.SENTINEL) for a in st.arrays}
    cur = S.prefix(table, min(n, period))                      # what the reference sees: one period of a tiled case
    blocks, capped = S.step_blocks(n)
    for launch in range(1, n_launches + 1):
        what = '%s %s n=%d off=%d (%d blocks%s) launch %d' % (st.entry, cfg, n, off, blocks, ', capped' if capped else '', launch)
        call(st.entry, *[bufs[a].ptr() for a in st.arrays], n, *S.step_floats(name, h), K().stream())
        got = {a: bufs[a].get() for a in S.outputs_of(name)}
        ref = S.step_ref(name, cur, h)
        assert ref.kink is None or not ref.kink.any(), what + ': an element of the table lies within its bound of the l1 kink'
        for arr, r in S.step_ratios(name, cfg, got, ref).items():
            within(r, '%s %s%s' % (what, arr, ' (exact)' if S.is_exact(name, cfg, arr) else ''))
        exact(bits(bufs['g'].get()), bits(inp['g']), what + ': g untouched')
        cur = dict({a: v[:len(cur['g'])] for a, v in got.items()}, g=cur['g'])      # the next reference starts from the device's outputs


STEP_IDS = ['n%d%s' % (n, '-off%d' % o if o else '') for n, o in S.STEP_CASES]


@pytest.mark.parametrize('n,off', S.STEP_CASES, ids=STEP_IDS)
@pytest.mark.parametrize('cfg', S.CFGS)
@pytest.mark.parametrize('name', S.STEP_NAMES)
def test_step(name, cfg, n, off):
    """Two launches in a row, every output array per element.  'exact': the accumulators (everything, for the momentum step)
    bit for bit; 'train': all by bound, from the slots engine.py creates.  ftrl_l1 runs FTRL with l1 = 0.25, l2 = 0.125."""
    run_step(name, cfg, n, off)


@pytest.mark.parametrize('name', S.BIG_STEPS)
def test_step_past_the_block_cap(name):
    """n = 4 * (4096 * 512) + 1200: ew_blocks() caps the grid at 4096 blocks, the grid-stride loop takes two more trips, the
    last ragged.  The 'exact' table (every slot varies) tiled with a period that puts each trip out of step with the last."""
    assert S.step_blocks(S.STEP_BIG_N)[1]
    run_step(name, 'exact', S.STEP_BIG_N, 0, n_launches=1, period=S.BIG_PERIOD)


def test_adam_step_past_the_block_cap():
    """tdg_adam_step at the same length, against adam_ref of tests/_exact_pointwise.py on a tiled table."""
    n, t = S.STEP_BIG_N, S.BIG_PERIOD
    small = P.adam_inputs(t)
    order = ('p', 'g', 'm', 'v')
    bufs = {a: Vec(n, 0, np.resize(getattr(small, a), n), fill=P.NAN if a == 'g' else P.SENTINEL) for a in order}
    lr_t = P.adam_lr_t(1, on_host=True)
    call('tdg_adam_step', *[bufs[a].ptr() for a in order], n, float(lr_t.v), P.ADAM.b1, P.ADAM.b2, P.ADAM.eps, P.ADAM.gs, K().stream())
    ref = P.adam_ref(small, lr_t)
    for a in ('m', 'v', 'p'):
        x = getattr(ref, a)
        within(S.tiled_ratio(bufs[a].get(), x.v, x.e), 'tdg_adam_step n=%d (capped) %s' % (n, a))
    exact(bits(bufs['g'].get()), bits(np.resize(small.g, n)), 'tdg_adam_step: g untouched')


@pytest.mark.parametrize('name', [k for k in S.STEP_NAMES if k != 'ftrl_l1'])
def test_step_argument_checks(name):
    """n not a multiple of 4, n = 0 and each pointer NULL are refused under the entry's own name; so is lr <= 0 by FTRL.
    A refused call writes nothing."""
    st, h = S.STEPS[name], S.hyper(name, 'train')
    inp = S.prefix(S.step_inputs(name, 'train'), 8)
    bufs = {a: Vec(8, 0, inp[a], fill=P.NAN if a == 'g' else P.SENTINEL) for a in st.arrays}
    ptrs = [bufs[a].ptr() for a in st.arrays]
    floats = S.step_floats(name, h)
    for n in (6, 7, 0):
        refused(st.entry, *ptrs, n, *floats, K().stream())
    for i in range(len(ptrs)):
        refused(st.entry, *(ptrs[:i] + [None] + ptrs[i + 1:]), 8, *floats, K().stream())
    if name == 'ftrl':
        for lr in (0.0, -0.1):
            refused(st.entry, *ptrs, 8, lr, *floats[1:], K().stream())
    for a in st.arrays:
        exact(bits(bufs[a].get()), bits(inp[a]), '%s: a refused call writes nothing (%s)' % (st.entry, a))


# ------------------------------------------------------------------------------------------------ 2. Philox draws
def draw(kind, seed, sid, offset, n, off=0, counter=None):
    """One launch of the host-offset form, or with `counter` (a device int32) of the _dev form: the n values."""
    dtype = 1 if kind == 'normal_bf16' else 0
    out = Vec(n, off, dtype=dtype)
    if kind == 'uniform':
        if counter is None:
            call('tdg_random_uniform_f32', seed, sid, offset, n, out.ptr(), K().stream())
        else:
            call('tdg_random_uniform_f32_dev', seed, sid, K().ptr(counter), n, out.ptr(), K().stream())
    elif counter is None:
        call('tdg_random_normal', dtype, seed, sid, offset, n, out.ptr(), K().stream())
    else:
        call('tdg_random_normal_dev', dtype, seed, sid, K().ptr(counter), n, out.ptr(), K().stream())
    return out.get()


def check_draw(kind, got, seed, sid, offset, n, what):
    """uniform: bit for bit; normal: per element within the bound of the Box-Muller chain."""
    blocks, capped, level = S.rng_blocks(n)
    what = '%s n=%d offset=%#x (%d blocks%s, %s tickets) %s' % (kind, n, offset, blocks, ', capped' if capped else '', level, what)
    if kind == 'uniform':
        exact(got, S.uniform_ref(seed, sid, offset, n), what)
        assert got.min() >= 0 and got.max() < 1
    else:
        ref, bound = S.normal_ref(seed, sid, offset, n, 1 if kind == 'normal_bf16' else 0)
        within(S.bound_ratio(got, ref, bound), what)


KINDS = ('uniform', 'normal', 'normal_bf16')


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('case', S.RNG_CASES, ids=S.RNG_IDS)
def test_draw_at_host_offset(case, kind):
    """The tail (n % 4 != 0), 64 and 66 blocks, the base one element off, a seed and a stream with their high words set, a
    counter that carries into its high word in mid-launch and one that starts there."""
    seed, sid, offset, n, off = case
    check_draw(kind, draw(kind, seed, sid, offset, n, off), seed, sid, offset, n, 'off=%d' % off)


@pytest.mark.parametrize('kind', KINDS)
def test_draw_past_the_block_cap(kind):
    """n = 4 * (4096 * 256) + 6: the grid is capped, the loop takes a second trip with a tail.  The host form against the
    reference, then the _dev form at draw 0 against the host form (the same counters), bit for bit."""
    seed, sid, n = S.SEED, (S.SID_UNIFORM if kind == 'uniform' else S.SID_NORMAL), S.RNG_BIG_N
    assert S.rng_blocks(n)[1] and S.draw_offset(0) == S.RNG_BIG_OFFSET
    host = draw(kind, seed, sid, S.RNG_BIG_OFFSET, n)
    check_draw(kind, host, seed, sid, S.RNG_BIG_OFFSET, n, 'host form')
    counter = torch.tensor([0, 77], dtype=torch.int32, device=dev())
    exact(bits(draw(kind, seed, sid, 0, n, counter=counter)), bits(host), kind + ' past the cap: _dev form against host form')
    assert counter.tolist() == [1, 77]


@pytest.mark.parametrize('order', S.DEV_ORDERS, ids=['-'.join(o) for o in S.DEV_ORDERS])
@pytest.mark.parametrize('d', S.DEV_DRAWS)
def test_dev_draws_count_and_match_the_host_form(d, order):
    """With the counter preset to d: each launch is bit-identical to the host form at offset (d + 1) << 24 (which first needs
    the counter's high word at d = 255), that host form matches the reference, and the counter rises by exactly one per
    launch -- three launches in a row that mix the two kernels and both ticket levels, all on the stream the rest of the
    suite uses for ticketed kernels."""
    counter = torch.tensor([d, 77, 77], dtype=torch.int32, device=dev())
    for i, (kind, n) in enumerate(zip(order, S.DEV_SIZES)):
        sid = S.SID_UNIFORM if kind == 'uniform' else S.SID_NORMAL
        got = draw(kind, S.SEED_HI, sid, 0, n, counter=counter)
        assert counter.tolist() == [d + i + 1, 77, 77], (kind, n, d)
        offset = S.draw_offset(d + i)
        host = draw(kind, S.SEED_HI, sid, offset, n)
        exact(bits(got), bits(host), '%s n=%d: _dev form at draw %d against the host form at offset %#x' % (kind, n, d + i, offset))
        check_draw(kind, host, S.SEED_HI, sid, offset, n, 'draw %d' % (d + i))
    assert counter.tolist() == [d + 3, 77, 77]


@pytest.mark.parametrize('kind', ['uniform', 'normal_bf16'])
def test_dev_draw_of_the_whole_window(kind):
    """n == 2**26, the whole window of a draw, stays legal: the first and the last counters' values match the reference, the
    last one being the counter in front of the next draw's first."""
    n, d, k = S.DRAW_WINDOW, 7, 8
    sid = S.SID_UNIFORM if kind == 'uniform' else S.SID_NORMAL
    dtype = 1 if kind == 'normal_bf16' else 0
    counter = torch.tensor([d, 77], dtype=torch.int32, device=dev())
    out = torch.full((n + TAIL,), P.SENTINEL, dtype=K().TORCH_DTYPE[dtype], device=dev())
    if kind == 'uniform':
        call('tdg_random_uniform_f32_dev', S.SEED, sid, K().ptr(counter), n, K().ptr(out), K().stream())
    else:
        call('tdg_random_normal_dev', dtype, S.SEED, sid, K().ptr(counter), n, K().ptr(out), K().stream())
    assert counter.tolist() == [d + 1, 77]
    assert np.all(out[n:].float().cpu().numpy() == P.SENTINEL)
    last = S.draw_offset(d) + n // 4 - k // 4
    assert last + k // 4 == S.draw_offset(d + 1)
    check_draw(kind, out[:k].float().cpu().numpy(), S.SEED, sid, S.draw_offset(d), k, 'the window\'s first values')
    check_draw(kind, out[n - k:n].float().cpu().numpy(), S.SEED, sid, last, k, 'the window\'s last values')
