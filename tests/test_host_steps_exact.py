"""The recipe of tests/_exact_steps.py checked on the CPU with reference arithmetic only: the NumPy Philox4x32-10 gives the
published known answers; for every exact output of the optimizer tables the terms and their sums are representable; for
every bounded output the reference is finite and the bound positive and finite, the centered root's argument stays
positive and no FTRL element sits on the kink; the tables reach every branch they were built for; float32 NumPy
restatements of the kernels are accepted clean and rejected with one named defect each, on the tables' own inputs; and
the reference streams are distinct where a dropped word would make them equal.  The one entry-point change, the draw
window of the _dev forms, is refused here too: argument checks run before anything is launched."""
import ctypes
import inspect

import numpy as np
import pytest

from conftest import pkg
import _exact_pointwise as P
import _exact_steps as S

LAUNCHES = (1, 2)
N = 2052                                   # the longest case the GPU file runs untiled


def launches(name, cfg, n=N):
    """(launch, inputs, hyper-parameters, reference) of two launches in a row; the second starts from the float32
    restatement's outputs, as the GPU file's second reference starts from the device's."""
    h = S.hyper(name, cfg)
    inp = S.prefix(S.step_inputs(name, cfg), n)
    for launch in LAUNCHES:
        yield launch, inp, h, S.step_ref(name, inp, h)
        inp = dict(S.restate_step(name, inp, h), g=inp['g'])


def words(*w):
    return [np.uint64(x) for x in w]


# ------------------------------------------------------------------------------------------------ Philox
KNOWN_ANSWERS = [      # (counter words, key words, output words): the Random123 known-answer file for philox4x32-10
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


def test_philox_known_answers():
    for c, k, want in KNOWN_ANSWERS:
        assert tuple(int(x) for x in S.philox_words(words(*c), words(*k))) == want
        # the same through the 64-bit interface: c = (ctr lo, ctr hi, stream lo, stream hi), k = (seed lo, seed hi)
        got = S.philox(k[0] | k[1] << 32, c[2] | c[3] << 32, c[0] | c[1] << 32, 1)[0]
        assert tuple(int(x) for x in got) == want
    many = S.philox(S.SEED, S.SID_NORMAL, 5, 7)
    assert many.shape == (7, 4) and np.array_equal(many[3], S.philox(S.SEED, S.SID_NORMAL, 8, 1)[0])     # each counter yields its own 4 words
    for d in S.PHILOX_DEFECTS[:2] + S.PHILOX_DEFECTS[3:]:
        assert tuple(int(x) for x in S.philox_words(words(*KNOWN_ANSWERS[2][0]), words(*KNOWN_ANSWERS[2][1]), d)) != KNOWN_ANSWERS[2][2]


def test_constants():
    L = pkg('_lib')
    assert (S.F32, S.BF16) == (L.F32, L.BF16) and S.SIN_ULP == S.COS_ULP == 4
    assert S.DRAW_WINDOW == 4 << 24 and S.draw_offset(0) == S.RNG_BIG_OFFSET and S.TWO_PI == float(np.float32(2 * np.pi))
    E = pkg('engine')
    dflt = lambda cls, k: inspect.signature(cls.__init__).parameters[k].default             # noqa: E731
    t = S.hyper('rmsprop', 'train')
    assert (t.decay, t.eps, t.mu) == (dflt(E.RMSProp, 'decay'), dflt(E.RMSProp, 'eps'), 0.3)
    t = S.hyper('adadelta', 'train')
    assert (t.rho, t.eps) == (dflt(E.Adadelta, 'rho'), dflt(E.Adadelta, 'eps'))
    assert np.all(S.step_inputs('adagrad', 'train')['acc'] == np.float32(dflt(E.Adagrad, 'initial_accumulator_value')))
    assert np.all(S.step_inputs('ftrl', 'train')['acc'] == np.float32(dflt(E.Ftrl, 'initial_accumulator_value')))
    assert np.all(S.step_inputs('rmsprop', 'train')['rms'] == 1) and np.all(S.step_inputs('rmsprop_centered', 'train')['mg'] == 0)
    for name in S.STEP_NAMES:
        assert set(S.step_inputs(name, 'exact')) == set(S.STEPS[name].arrays) == set(S.step_inputs(name, 'train'))
        assert L.SIGNATURES[S.STEPS[name].entry][1].count(L._f) == len(S.STEPS[name].floats) + 1
    h = S.hyper('ftrl_l1', 'train')
    assert (h.l1, h.l2) == (0.25, 0.125) and (S.hyper('ftrl', 'train').l1, S.hyper('ftrl', 'train').l2) == (0, 0)


# ------------------------------------------------------------------------------------------------ exact outputs
def exact_terms(name, inp, h):
    """Every f32 intermediate on the way to the kernel's exact outputs, in float64."""
    g = inp['g'].astype(np.float64)
    gv = S.GS * g
    x = {k: v.astype(np.float64) for k, v in inp.items()}
    if name.startswith('rmsprop'):
        t = [gv, h.decay * x['rms'], (1 - h.decay) * gv, (1 - h.decay) * gv * gv]
        return t + ([h.decay * x['mg']] if name == 'rmsprop_centered' else [])
    if name == 'adadelta':
        return [gv, h.rho * x['acc'], (1 - h.rho) * gv, (1 - h.rho) * gv * gv]
    if name == 'sgd':
        a = h.mu * x['acc'] + gv
        return [gv, h.mu * x['acc'], a, h.lr * a]
    return [gv, gv * gv]


@pytest.mark.parametrize('name', S.STEP_NAMES)
def test_exact_outputs_are_representable(name):
    """Two launches in a row: every term fits f32, the terms lie on a 2**-12 grid (but for the two 2**-20 gradients of the
    rmsprop table) with sums far below 2**24 grid steps, and every exact output fits f32 -- so the device must give those
    bits with or without fused multiply-adds."""
    h = S.hyper(name, 'exact')
    for k in ('lr', 'decay', 'mu', 'rho'):
        assert np.log2(getattr(h, k)) == round(np.log2(getattr(h, k)))
    assert S.STEPS[name].exact
    for launch, inp, _, ref in launches(name, 'exact'):
        assert all(S.fits_f32(v) for v in inp.values())
        terms = exact_terms(name, inp, h)
        assert all(S.fits_f32(t) for t in terms), (name, launch)
        coarse = np.ones(N, dtype=bool)
        if name == 'rmsprop':
            coarse[list(S.TINY_AT)] = False
            assert all(inp['rms'][i] <= 2.0 ** -40 and inp['g'][i] == 2.0 ** -20 for i in S.TINY_AT)
        for t in terms:
            assert np.array_equal(np.rint(t[coarse] * 4096), t[coarse] * 4096), (name, launch)
        S.on_grid(sum(np.abs(t[coarse]) for t in terms), 2.0 ** -12, '%s launch %d' % (name, launch))
        for arr in S.STEPS[name].exact:
            assert S.fits_f32(ref.out[arr].v), (name, arr, launch)
            assert np.array_equal(S.restate_step(name, inp, h)[arr], S.store(ref.out[arr].v, S.F32))


# ------------------------------------------------------------------------------------------------ bounded outputs
@pytest.mark.parametrize('cfg', S.CFGS)
@pytest.mark.parametrize('name', S.STEP_NAMES)
def test_bounded_outputs_have_finite_references_and_positive_bounds(name, cfg):
    for launch, inp, h, ref in launches(name, cfg, S.TABLE):
        assert set(ref.out) == set(S.outputs_of(name))
        for arr, x in ref.out.items():
            zero = (x.v == 0) if (name, arr) == ('ftrl_l1', 'p') else np.zeros(len(x.v), dtype=bool)      # the branch's 0.f: exact
            assert np.all(np.isfinite(x.v)) and np.all(np.isfinite(x.e)) and np.all((x.e > 0) | zero), (name, cfg, arr, launch)
        if name == 'rmsprop_centered':
            assert np.all(inp['rms'].astype(np.float64) >= inp['mg'].astype(np.float64) ** 2 + (0.25 if launch == 1 else 0.1))
            assert np.all(ref.root.v - ref.root.e > 0.1)                    # the square root's argument stays clear of 0
        if name.startswith('ftrl'):
            assert int(ref.kink.sum()) == 0, '%s %s launch %d: %d elements lie within their bound of l1' % (name, cfg, launch, ref.kink.sum())
            lin, p = ref.out['linear'].v, ref.out['p'].v
            if name == 'ftrl_l1':
                on = np.abs(lin) > h.l1
                for m in (on, ~on, on & (lin < 0), on & (lin > 0), inp['g'] == 0, ~on & (lin != 0)):
                    assert m[:N].sum() >= 8, (cfg, launch)
                assert np.all(p[~on] == 0) and np.all(p[on] != 0) and np.all(ref.out['p'].e[~on] == 0)
            else:
                assert np.all(lin != 0) and np.all(p != 0)


def test_generators_are_deterministic():
    for name in S.STEP_NAMES:
        for cfg in S.CFGS:
            a, b = S.step_inputs(name, cfg), S.step_inputs(name, cfg)
            assert all(np.array_equal(a[k], b[k]) and a[k].dtype == np.float32 and len(a[k]) == S.TABLE for k in a)
    t = S.step_inputs('sgd', 'train')
    big = S.prefix(t, 3 * S.BIG_PERIOD + 8, S.BIG_PERIOD)
    assert np.array_equal(big['p'][S.BIG_PERIOD:2 * S.BIG_PERIOD], t['p'][:S.BIG_PERIOD]) and np.array_equal(big['p'][-8:], t['p'][:8])
    assert np.array_equal(S.prefix(t, 4)['g'], t['g'][:4])


# ------------------------------------------------------------------------------------------------ branches
def test_tables_reach_every_branch():
    assert [S.step_blocks(n) for n, _ in S.STEP_CASES] == [(1, False), (2, False), (2, False)] and [o for _, o in S.STEP_CASES] == [0, 0, 4]
    assert S.step_blocks(S.STEP_BIG_N) == (4096, True) and S.STEP_BIG_N == 4 * (4096 * 512) + 4 * 300
    trip = 4096 * 256                                                    # vectors per trip of the capped grid (256 threads a block)
    assert divmod(S.STEP_BIG_N // 4, trip) == (2, 300)                   # two full trips, then a ragged one that two blocks take
    assert divmod((S.RNG_BIG_N + 3) // 4, trip) == (1, 2)
    assert S.BIG_PERIOD % 4 == 0 and (4 * 4096 * 256) % S.BIG_PERIOD == 4 and S.BIG_PERIOD >= max(S.TINY_AT) + 1
    assert all(n % 4 == 0 for n, _ in S.STEP_CASES) and set(S.BIG_STEPS) | {'ftrl'} == set(S.STEP_NAMES)
    assert [S.rng_blocks(n) for n in S.RNG_N] == [(1, False, 'one-level')] * 4 + [(64, False, 'one-level'), (66, False, 'two-level')]
    assert S.rng_blocks(S.RNG_BIG_N) == (4096, True, 'two-level') and S.RNG_BIG_N % 4 and S.RNG_BIG_N <= S.DRAW_WINDOW
    assert sorted(n % 4 for n in S.RNG_N[:4]) == [0, 1, 1, 3]
    # every _dev entry meets both ticket levels, and three launches in a row mix the two kernels
    level = {}
    for order in S.DEV_ORDERS:
        assert len(set(k.split('_')[0] for k in order)) == 2
        for kind, n in zip(order, S.DEV_SIZES):
            level.setdefault(kind.split('_')[0], set()).add(S.rng_blocks(n)[2])
    assert level == {'normal': {'one-level', 'two-level'}, 'uniform': {'one-level', 'two-level'}}
    assert any('bf16' in k for order in S.DEV_ORDERS for k in order)
    # keys and counters that reach every word
    hi = lambda v: v >> 32                                                                  # noqa: E731
    assert any(hi(c[0]) for c in S.RNG_CASES) and any(hi(c[1]) for c in S.RNG_CASES) and any(c[4] for c in S.RNG_CASES)
    assert any(not hi(c[2]) and hi(c[2] + (c[3] + 3) // 4 - 1) for c in S.RNG_CASES)         # the carry, in mid-launch
    assert any(c[2] == 257 << 24 for c in S.RNG_CASES)
    assert [hi(S.draw_offset(d)) > 0 for d in S.DEV_DRAWS] == [False, False, True, True, True] and max(S.DEV_DRAWS) + 3 < 2 ** 31


# ------------------------------------------------------------------------------------------------ mutation checks
@pytest.mark.parametrize('cfg', S.CFGS)
@pytest.mark.parametrize('name', S.STEP_NAMES)
def test_steps_restated_clean_and_with_one_defect(name, cfg):
    """The clean restatement passes the comparison the device's result gets, at both launches; each named defect fails
    it.  sqrtf(rms) + eps differs from sqrtf(rms + eps) by 1e-10 at the training defaults, far inside any f32 bound: it is
    the 'exact' table's two elements with rms = 0 and g = 2**-20 that reject it."""
    for launch, inp, h, ref in launches(name, cfg):
        assert S.accepted(S.step_ratios(name, cfg, S.restate_step(name, inp, h), ref)), (name, cfg, launch)
        for defect in S.STEP_DEFECTS[name]:
            r = S.step_ratios(name, cfg, S.restate_step(name, inp, h, defect), ref)
            if defect == 'eps_outside_root' and cfg == 'train':
                continue
            assert not S.accepted(r), (name, cfg, launch, defect)
            if defect == 'one_vector_short':
                assert all(np.all(v[:-4] <= 1) and np.all(v[-4:] > 1) for v in r.values())
    # the big case's comparison: a tiling of the period is accepted, one element off is not
    h, table = S.hyper(name, cfg), S.step_inputs(name, cfg)
    small = S.prefix(table, S.BIG_PERIOD)
    ref = S.step_ref(name, small, h)
    n = 2 * S.BIG_PERIOD + 12
    got = {k: np.resize(v, n) for k, v in S.restate_step(name, small, h).items()}
    assert S.accepted(S.step_ratios(name, cfg, got, ref))
    got['p'][-1] += 1.0
    assert not S.accepted(S.step_ratios(name, cfg, got, ref))


def all_offsets():
    return [c[:4] for c in S.RNG_CASES] + [(S.SEED, S.SID_UNIFORM, S.draw_offset(d), 9) for d in S.DEV_DRAWS]


def test_uniform_restated_clean_and_with_one_defect():
    for seed, sid, offset, n in all_offsets():
        want = S.uniform_ref(seed, sid, offset, n)
        assert want.dtype == np.float32 and len(want) == n and np.all(want >= 0) and np.all(want < 1)
        assert S.fits_f32(S.u01(S.philox(seed, sid, offset, (n + 3) // 4)))
        for defect in S.PHILOX_DEFECTS + ('shift_9',):
            same = np.array_equal(S.uniform_ref(seed, sid, offset, n, defect), want)
            high = (offset + (n + 3) // 4 - 1) >> 32 > 0
            blind = (defect == 'counter_high_dropped' and not high) or (defect == 'words_1_3_swapped' and n == 1)    # (one value: word 0 alone)
            assert same == blind, (hex(offset), n, defect)


@pytest.mark.parametrize('dtype', [0, 1])
def test_normal_restated_clean_and_with_one_defect(dtype):
    ok = lambda got, ref, bound: bool(np.all(S.bound_ratio(got, ref, bound) <= 1.0))          # noqa: E731
    for seed, sid, offset, n in all_offsets():
        ref, bound = S.normal_ref(seed, sid, offset, n, dtype)
        assert np.all(np.isfinite(ref)) and np.all(np.isfinite(bound)) and np.all(bound > 0) and len(ref) == n
        assert ok(S.restate_normal(seed, sid, offset, n, dtype), ref, bound), (hex(offset), n)
        for defect in S.PHILOX_DEFECTS + ('u1_is_u01',):
            high = (offset + (n + 3) // 4 - 1) >> 32 > 0
            rejected = not ok(S.restate_normal(seed, sid, offset, n, dtype, defect), ref, bound)
            assert rejected == (defect != 'counter_high_dropped' or high), (hex(offset), n, defect)


def test_box_muller_at_the_ends_of_u1():
    """A first word below 256 gives u1 = 1 and the value 0; a first word of all ones gives u1 = 2**-24 and a finite value."""
    z = S.box_muller(np.uint32([[0, 1 << 30, 255, 3 << 30], [0xffffffff, 0, 0xffffff00, 1 << 31]]), 8)
    assert np.all(z.v[:4] == 0) and np.all(z.e[:4] < 1e-18)
    r = np.sqrt(2 * 24 * np.log(2.0))
    assert np.allclose(z.v[4:], [r, 0, -r, 0], atol=1e-6) and np.all(np.isfinite(z.e)) and np.all(z.e[4:] < 1e-5)


# ------------------------------------------------------------------------------------------------ distinctness
def test_reference_streams_are_distinct():
    """What the table could not tell apart, it could not test: the two streams of a rank, draw windows 256 apart (equal if
    the counter's high word were dropped) and neighbouring counters all differ, in every word."""
    n = 64
    differ = lambda a, b: bool(np.all(a != b))                                               # noqa: E731 (word for word)
    for rank in (0, 1, 3):
        a, b = (S.philox(S.SEED, (rank << 8) | k, S.draw_offset(0), n) for k in (1, 2))
        assert differ(a, b)
    assert differ(S.philox(S.SEED, 1, 0, n), S.philox(S.SEED, 1 << 8 | 1, 0, n))              # rank 0 and rank 1
    for d in S.DEV_DRAWS:
        assert differ(S.philox(S.SEED, S.SID_NORMAL, S.draw_offset(d), n), S.philox(S.SEED, S.SID_NORMAL, S.draw_offset(d + 256), n))
        assert differ(S.philox(S.SEED, S.SID_NORMAL, S.draw_offset(d), n), S.philox(S.SEED, S.SID_NORMAL, S.draw_offset(d + 1), n))
    w = S.philox(S.SEED, S.SID_NORMAL, 2 ** 32 - 32, n)
    assert differ(w[1:], w[:-1]) and len(np.unique(w)) == w.size
    assert differ(S.philox(S.SEED, S.SID_NORMAL, 0, n), S.philox(S.SEED_HI, S.SID_NORMAL, 0, n))
    assert differ(S.philox(S.SEED, S.SID_NORMAL, 0, n), S.philox(S.SEED | 1 << 32, S.SID_NORMAL, 0, n))       # the key's high word alone
    assert differ(S.philox(S.SEED, S.SID_NORMAL, 0, n), S.philox(S.SEED, S.SID_NORMAL | 1 << 32, 0, n))      # the stream's high word alone
    # a draw of the window's full length ends one counter short of the next draw's first
    assert S.draw_offset(0) + S.DRAW_WINDOW // 4 == S.draw_offset(1)


# ------------------------------------------------------------------------------------------------ the draw window
def test_dev_draws_refuse_more_than_their_window():
    """n > 2**26 would run into the next draw's counters: TDG_EINVAL with the entry's name and the window in the message,
    before anything is launched (the pointers are host memory that is never touched)."""
    lib = pkg('_lib').load()
    buf = (ctypes.c_float * 8)()
    ptr = ctypes.cast(buf, ctypes.c_void_p)
    for n in (S.DRAW_WINDOW + 1, 1 << 40):
        for name, args in (('tdg_random_normal_dev', (0, 1, 1, ptr, n, ptr, None)), ('tdg_random_uniform_f32_dev', (1, 1, ptr, n, ptr, None))):
            assert getattr(lib, name)(*args) == -1
            msg = lib.tdg_last_error().decode()
            assert msg.startswith(name + ':') and 'window' in msg and str(S.DRAW_WINDOW) in msg and str(n) in msg, msg
    assert not any(buf)
