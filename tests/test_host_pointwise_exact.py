"""The recipe of tests/_exact_pointwise.py checked on the CPU with reference arithmetic only: for every exact case of the
tables tests/test_gpu_pointwise_exact.py runs, the representability conditions hold on reference values; for every
bounded case the reference is finite and the bound positive and finite; the generators are deterministic; the tables
reach every branch they were built for; and NumPy restatements of the kernels are accepted clean and rejected with one
named defect each, on the tables' own inputs."""
import numpy as np
import pytest

from conftest import pkg
import _exact_pointwise as P


def rep(v, dtype=1):
    """Every value is representable in the storage type."""
    v = np.atleast_1d(np.asarray(v, dtype=np.float64))
    return bool(np.array_equal(P.store(v, dtype).astype(np.float64), v))


def good_bound(ref, bound):
    return bool(np.all(np.isfinite(ref)) and np.all(np.isfinite(bound)) and np.all(np.asarray(bound) > 0))


def accepted(got, ref, bound, dtype=0):
    """The comparison of the GPU file: exact against store(ref) where bound is None, else every ratio <= 1."""
    if bound is None:
        return bool(np.array_equal(got, P.store(ref, dtype)))
    return bool(np.all(P.bound_ratio(got, ref, bound) <= 1.0))


def test_constants_match_the_library():
    L = pkg('_lib')
    assert P.ACTS == (L.ACT_NONE, L.ACT_RELU, L.ACT_LRELU, L.ACT_TANH, L.ACT_SIGMOID)
    assert (P.F32, P.BF16) == (L.F32, L.BF16) and (L.MASK_NONE, L.MASK_LRELU, L.MASK_RELU) == (0, 1, 2)
    assert P.LEAK == 0.25 and rep(P.SENTINEL) and P.TANH_ULP == 5
    assert np.array_equal(P.bf16_round(P.TIES), P.TIES_BF16)
    assert P.bf16_round(np.float32([1 + 2.0 ** -8]))[0] == 1.0 and P.bf16_round(np.float32([1 + 3 * 2.0 ** -8]))[0] == 1 + 2.0 ** -6


# ------------------------------------------------------------------------------------------------ exact cases
@pytest.mark.parametrize('n', P.FLAT_N + (P.BIG_N,))
def test_flat_cases_are_exact(n):
    inp = P.add_act_inputs(n)
    assert rep(inp.a) and rep(inp.b)
    for act in P.EXACT_ACTS:
        ref, bound = P.add_act_ref(inp, act, 1)
        assert bound is None and rep(ref)
    assert rep(P.affine_inputs(n)) and rep(P.affine_ref(P.affine_inputs(n))) and rep(P.affine_inputs(n).astype(np.float64) + P.AFFINE_SHIFT, 0)
    if n == P.BIG_N:
        return
    b = P.act_bwd_inputs(n)
    assert rep(b.dy) and rep(b.post)
    for act in P.ACTS:
        r = P.act_bwd_ref(b, act)
        assert rep(r.f, 0) and rep(r.dx) and rep(b.post.astype(np.float64) ** 2, 0)
    if n >= 255:
        z = b.post == 0
        assert np.signbit(b.post[z]).any() and not np.signbit(b.post[z]).all()              # +0.0 and -0.0
        assert np.all(P.act_bwd_ref(b, P.ACT_RELU).dx[z] == 0) and np.all(P.act_bwd_ref(b, P.ACT_LRELU).f[z] == P.LEAK)
    x = P.scale_inputs(n).x
    assert all(rep(k * x.astype(np.float64)) for k in P.SCALE_COEFS) and rep(P.cast_inputs(n).x)
    for lo, hi in P.CLAMPS:
        c = P.clamp_inputs(n, lo, hi)
        if n >= 8:
            assert (c == lo).any() and (c == hi).any() and (c < lo).any() and (c > hi).any()
    assert rep(P.FILL_VALUE, 0)


def test_strided_cases_are_exact():
    for rows, c in P.BIAS_ACT_SHAPES:
        inp = P.bias_act_inputs(rows, c)
        assert P.strides_of(c)[0] == c and len(P.strides_of(c)) >= 2
        for act in P.EXACT_ACTS:
            for wb in (False, True):
                ref, bound = P.bias_act_ref(inp, wb, act, 1)
                assert bound is None and rep(ref)
    for rows in P.CAST_ROWS_ROWS:
        for c in P.CAST_ROWS_C:
            assert rep(P.affine_ref(P.affine_inputs((rows, c))))
    for keep in P.DROPOUT_KEEPS:
        for c in P.DROPOUT_C:
            inp = P.dropout_inputs(c, keep)
            once = P.dropout_ref(inp.y, inp.u, keep)
            assert rep(inp.y) and rep(keep + inp.u.astype(np.float64), 0) and rep(once) and rep(inp.y.astype(np.float64) / keep ** 2)
            assert np.all(inp.y != 0) and once.ravel()[0] != 0 and (keep == 1 or (once.ravel()[1] == 0 and once.ravel()[2] == 0))
            assert keep == 1 or ((once == 0).any() and (once != 0).any())
    for rows in P.GP_INTERP_ROWS:
        for cols in P.GP_INTERP_COLS:
            inp = P.gp_interp_inputs(rows, cols)
            x, g, al = inp.x.astype(np.float64), inp.g.astype(np.float64), inp.alpha.astype(np.float64)[:, None]
            assert rep(inp.x) and rep(inp.g) and rep(g - x, 0) and rep(al * (g - x), 0) and rep(P.gp_interp_ref(inp))
            assert inp.alpha[0] == 0 and (rows == 1 or inp.alpha[1] == 1)
    for c in P.JOIN_C:
        inp = P.join_inputs(c, 6)
        assert rep(inp.comb) and rep(P.join_fwd_ref(inp)) and all(rep(v) for v in P.join_bwd_ref(inp))
        s = P.join_strides(c)
        assert len(set(s) | {c}) == 4 and all(v % 8 == 0 for v in s) and s[0] >= 2 * c


def test_vae_and_loss_exact_cases():
    for L in P.VAE_L:
        assert len(set(P.vae_strides(L))) == 3 and P.vae_strides(L)[0] > 2 * L and P.vae_strides(L)[1] > L and P.vae_strides(L)[2] > L
        for rows in P.VAE_ROWS:
            inp = P.reparam_inputs(rows, L)
            assert all(rep(a) for a in (inp.m, inp.sd, inp.eps, inp.dz))
            assert rep(inp.sd.astype(np.float64) * inp.eps, 0) and rep(P.reparam_ref(inp)) and rep(P.reparam_bwd_ref(inp))
    assert max(r * L for r in P.VAE_ROWS for L in P.VAE_L) > 256
    for rows, c in P.L1_CASES:
        inp = P.l1_inputs(rows, c)
        r = P.l1_ref(inp, 0)
        assert rep(inp.d) and rep(r.u, 0) and np.array_equal(r.u * 128, np.rint(r.u * 128))
        P.on_grid(r.sum, 1.0 / 128, 'sum |u|')
        assert rows * c == 1 or ((r.u == 0).any() and (r.u > 0).any() and (r.u < 0).any())
        assert r.pow2 == ((rows, c) in ((1, 1), (1024, 1)))
        if r.pow2:
            assert rep(r.loss, 0) and rep(r.inv_n)
    for rows in P.P2P_L1_ROWS:
        inp = P.p2p_l1_inputs(rows)
        r = P.p2p_l1_ref(inp, 0)
        assert rep(inp.y) and rep(inp.g) and rep(inp.dg) and (r.d == 0).any()
        P.on_grid(r.a, 0.5, 'sum |d|')
        P.on_grid(r.q, 0.25, 'sum d^2')
        assert r.pow2 == (rows in (1, 256))
        if r.pow2:
            assert rep(r.dg, 0) and rep(r.scal[0], 0)          # the f32 sum is exactly known; the bf16 store rounds it once
    for rows, cols in P.GP_ROWS_EXACT:
        r = P.gp_rows_ref(P.gp_rows_inputs(rows, cols), 1)
        assert rep(r.pen, 0) and rep(r.u) and int(round(np.sqrt(cols))) ** 2 == cols
        assert cols != 1 or (np.all(r.pen == 0) and np.all(r.u == 0))


# ------------------------------------------------------------------------------------------------ bounded cases
def test_bounded_cases_have_finite_references_and_positive_bounds():
    for dtype in (0, 1):
        for n in P.FLAT_N:
            for act in (P.ACT_TANH, P.ACT_SIGMOID):
                assert good_bound(*P.add_act_ref(P.add_act_inputs(n), act, dtype))
        for rows, c in P.BIAS_ACT_SHAPES:
            for act in (P.ACT_TANH, P.ACT_SIGMOID):
                assert good_bound(*P.bias_act_ref(P.bias_act_inputs(rows, c), True, act, dtype))
        for L in P.VAE_L:
            for rows in P.VAE_ROWS:
                inp = P.kl_inputs(rows, L)
                for klw in (0.0, 1.0):
                    assert good_bound(*P.reparam_bwd_kl_ref(inp, klw, dtype))
                assert rows * L < 9 or all((inp.sd == v).any() for v in (0.0, 2.0 ** -10, -2.0 ** -10))
        for rows in P.BCE_ROWS:
            for c in P.BCE_C:
                inp = P.bce_inputs(rows, c)
                r = P.bce_ref(inp, dtype)
                assert good_bound(r.loss, r.loss_bound) and good_bound(r.seed, r.seed_bound)
                assert inp.d.ravel()[0] == 0 and (rows == 1 or all((inp.d == v).any() for v in (0.0, 1.0, 2.0 ** -7, 0.5)))
        for rows in P.P2P_L1_ROWS:
            r = P.p2p_l1_ref(P.p2p_l1_inputs(rows), dtype)
            assert good_bound(r.dg, r.dg_bound) and good_bound(r.scal, r.scal_bound)
        for rows in P.XENT_ROWS:
            inp = P.xent_inputs(rows)
            assert rep(inp.z)
            assert all((np.abs(inp.z) == v).any() for v in ((88.0,) if rows == 1 else (0.0, 2.0 ** -10, 30.0, 88.0)))
            for mode in (0, 1, 2):
                r = P.xent_ref(inp, mode, dtype)
                assert good_bound(r.scal, r.scal_bound)
                if mode:
                    assert np.all(np.isfinite(r.seed)) and np.all(np.isfinite(r.seed_bound))
                    assert np.all(r.seed_bound[rows:] > 0) and (mode == 2) == bool(np.all(r.seed_bound[:rows] == 0))
        for rows, cols in P.GP_ROWS_BOUNDED:
            r = P.gp_rows_ref(P.gp_rows_inputs(rows, cols), dtype)
            assert good_bound(r.pen, r.pen_bound) and good_bound(r.u, r.u_bound)
    for rows, L in P.VAE_KL_SHAPES:
        inp = P.kl_inputs(rows, L)
        assert good_bound(*P.vae_kl_ref(inp)) and inp.m.ravel()[0] == 0 and inp.sd.ravel()[0] == 0
        assert rows * L == 1 or (inp.sd == 1).any()
    assert [r * L for r, L in P.VAE_KL_SHAPES] == [1, 257, 70000]
    for rows, c in P.L1_CASES:
        r = P.l1_ref(P.l1_inputs(rows, c), 0)
        assert r.pow2 or good_bound(r.loss, r.loss_bound)
    for n in P.LOGLOSS_N:
        inp = P.logloss_inputs(n)
        r = P.logloss_ref(inp)
        assert good_bound(r.scal, r.scal_bound) and all(good_bound(s.v, s.e) for s in r.seeds)
        assert n == 1 or all((inp.dr == v).any() and (inp.df == v).any() for v in (0.0, 1.0, 0.5, 2.0 ** -20))
    for n in P.ADAM_N:
        inp = P.adam_inputs(n)
        for t0 in P.ADAM_T0:
            for lr_t in (P.adam_lr_t(t0 + 1), P.adam_lr_t(t0 + 1, on_host=True)):
                r = P.adam_ref(inp, lr_t)
                assert all(good_bound(x.v, x.e) for x in (r.m, r.v, r.p))
        assert n % 4 == 0


def test_generators_are_deterministic():
    gens = [(P.add_act_inputs, (257,)), (P.act_bwd_inputs, (257,)), (P.bias_act_inputs, (3, 8)), (P.dropout_inputs, (7, 0.5)),
            (P.gp_interp_inputs, (3, 7)), (P.join_inputs, (8, 6)), (P.reparam_inputs, (3, 7)), (P.kl_inputs, (3, 7)), (P.bce_inputs, (257, 3)),
            (P.l1_inputs, (5, 3)), (P.p2p_l1_inputs, (257,)), (P.xent_inputs, (255,)), (P.logloss_inputs, (255,)), (P.gp_rows_inputs, (3, 7)),
            (P.adam_inputs, (2052,)), (P.cast_inputs, (257,))]
    for gen, args in gens:
        a, b = vars(gen(*args)), vars(gen(*args))
        assert all(np.array_equal(a[k], b[k], equal_nan=True) for k in a), gen.__name__
    assert np.array_equal(P.affine_inputs((3, 4)), P.affine_inputs((3, 4))) and np.array_equal(P.clamp_inputs(257, -1, 2), P.clamp_inputs(257, -1, 2))


# ------------------------------------------------------------------------------------------------ branches
def test_tables_reach_every_branch():
    assert {P.cast_rows_branch(c) for c in P.CAST_ROWS_C} == {'c<=16', 'c>16'} and 16 in P.CAST_ROWS_C and 17 in P.CAST_ROWS_C
    assert P.flat_blocks(P.BIG_N) == (4096, True) and not any(P.flat_blocks(n)[1] for n in P.FLAT_N)
    assert [P.flat_blocks(n)[0] for n in P.FLAT_N] == [1, 1, 1, 1, 2]
    assert [P.ticket_level(n) for n in P.ADAM_N] == [(1, 'one-level'), (2, 'one-level'), (64, 'one-level'), (65, 'two-level')]
    assert max(r for r, _ in P.BIAS_ACT_SHAPES) > 4096 and max(P.GP_INTERP_ROWS) > 4096 and max(r for r, _ in P.GP_ROWS_BOUNDED) > 4096
    assert max(P.BCE_ROWS) > 256 * 256 and max(P.P2P_L1_ROWS) > 256 * 256                    # a second trip of the two-stage reductions
    assert max(P.XENT_ROWS) > 256 and max(P.LOGLOSS_N) > 256                                # a second trip of the one-block ones
    assert set(P.ACTS) == {0, 1, 2, 3, 4} and set(P.EXACT_ACTS) | {P.ACT_TANH, P.ACT_SIGMOID} == set(P.ACTS)
    # the NULL arguments and the modes are loops of the GPU file over these tables
    assert {m for m, _ in P.XENT_RUNS} == {0, 1, 2} and (0, False) in P.XENT_RUNS and all(given or m == 0 for m, given in P.XENT_RUNS)
    assert set(P.DG_GIVEN) == {True, False} and set(P.BIAS_GIVEN) == {True, False}
    assert P.JOIN_RUNS == ((0, 6, True), (1, 6, True), (1, 3, False)) and P.JOIN_N_RGB == 3


# ------------------------------------------------------------------------------------------------ mutation checks
@pytest.mark.parametrize('dtype', [0, 1])
def test_affine_cast_rows_restated_clean_and_with_cs_for_c(dtype):
    for c in P.CAST_ROWS_C:
        x = P.affine_inputs((257, c))
        want = P.store(P.affine_ref(x), dtype)
        lay, out = P.restate_affine_cast_rows(x, c + 3, dtype)
        assert np.array_equal(lay.unpack(out), want) and np.all(lay.outside(out) == P.SENTINEL)
        lay, out = P.restate_affine_cast_rows(x, c + 3, dtype, 'cs_for_c')
        assert not np.array_equal(lay.unpack(out), want)


@pytest.mark.parametrize('dtype', [0, 1])
def test_padding_written_and_last_element_dropped_are_rejected(dtype):
    for rows, c in P.BIAS_ACT_SHAPES:
        inp = P.bias_act_inputs(rows, c)
        ref, _ = P.bias_act_ref(inp, True, P.ACT_LRELU, dtype)
        for cs in P.strides_of(c):
            lay, out = P.restate_bias_act(inp.x, inp.bias, cs, P.ACT_LRELU, dtype)
            assert np.array_equal(lay.unpack(out), P.store(ref, dtype)) and np.all(lay.outside(out) == P.SENTINEL)
            lay, out = P.restate_bias_act(inp.x, inp.bias, cs, P.ACT_LRELU, dtype, 'pad_written')
            assert np.all(lay.outside(out) == P.SENTINEL) == (cs == c)                      # the guard check of Buf.get()
    for n in P.FLAT_N:
        inp = P.add_act_inputs(n)
        ref, _ = P.add_act_ref(inp, P.ACT_RELU, dtype)
        lay, out = P.restate_add_act(inp.a, inp.b, P.ACT_RELU, dtype)
        assert np.array_equal(lay.unpack(out).ravel(), P.store(ref, dtype))
        lay, out = P.restate_add_act(inp.a, inp.b, P.ACT_RELU, dtype, 'drop_last')
        assert not np.array_equal(lay.unpack(out).ravel(), P.store(ref, dtype))             # the sentinel is no correct answer


def test_act_bwd_mask_at_zero():
    for n in P.FLAT_N[1:]:
        inp = P.act_bwd_inputs(n)
        for act in P.ACTS:
            want = P.store(P.act_bwd_ref(inp, act).dx, 0)
            assert np.array_equal(P.restate_act_bwd(inp.dy, inp.post, act), want)
            assert np.array_equal(P.restate_act_bwd(inp.dy, inp.post, act, 'ge_at_zero'), want) == (act not in (P.ACT_RELU, P.ACT_LRELU))


@pytest.mark.parametrize('dtype', [0, 1])
def test_l1_sign_of_zero_and_inv_n(dtype):
    for rows, c in P.L1_CASES:
        inp = P.l1_inputs(rows, c)
        ref = P.l1_ref(inp, dtype)
        loss, seed = P.restate_l1(inp.x, inp.d, dtype)
        assert np.array_equal(seed, P.store(ref.seed, dtype)) and accepted(loss, ref.loss, ref.loss_bound)
        if rows * c > 1:
            _, seed = P.restate_l1(inp.x, inp.d, dtype, 'sign0_is_1')
            assert not np.array_equal(seed, P.store(ref.seed, dtype))
        loss, seed = P.restate_l1(inp.x, inp.d, dtype, 'inv_rows')
        assert (np.array_equal(seed, P.store(ref.seed, dtype)) and accepted(loss, ref.loss, ref.loss_bound)) == (c == 1)


@pytest.mark.parametrize('dtype', [0, 1])
def test_xent_halves_swapped_and_dg_overwritten(dtype):
    for rows in P.XENT_ROWS:
        inp = P.xent_inputs(rows)
        for mode in (1, 2):
            ref = P.xent_ref(inp, mode, dtype)
            assert accepted(P.restate_xent_seeds(inp.z, mode, dtype), ref.seed, ref.seed_bound)
            assert not accepted(P.restate_xent_seeds(inp.z, mode, dtype, 'halves_swapped'), ref.seed, ref.seed_bound)
    for rows in P.P2P_L1_ROWS:
        inp = P.p2p_l1_inputs(rows)
        ref = P.p2p_l1_ref(inp, dtype)
        bound = None if ref.pow2 else ref.dg_bound
        assert accepted(P.restate_p2p_l1_dg(inp.y, inp.g, inp.dg, dtype), ref.dg, bound, dtype)
        assert not accepted(P.restate_p2p_l1_dg(inp.y, inp.g, inp.dg, dtype, 'overwrite'), ref.dg, bound, dtype)


@pytest.mark.parametrize('dtype', [0, 1])
def test_bce_guard_omitted(dtype):
    for rows in P.BCE_ROWS[:2]:
        for c in P.BCE_C:
            inp = P.bce_inputs(rows, c)
            ref = P.bce_ref(inp, dtype)
            assert accepted(P.restate_bce_seed(inp.x, inp.d, dtype), ref.seed, ref.seed_bound)
            assert not accepted(P.restate_bce_seed(inp.x, inp.d, dtype, 'no_guard'), ref.seed, ref.seed_bound)      # d == 0: x / 0


def test_adam_step_count_read_after_the_increment():
    for n in P.ADAM_N[:2]:
        inp = P.adam_inputs(n)
        for t0 in P.ADAM_T0:
            ref = P.adam_ref(inp, P.adam_lr_t(t0 + 1))
            p, m, v = P.restate_adam(inp, t0)
            assert accepted(p, ref.p.v, ref.p.e) and accepted(m, ref.m.v, ref.m.e) and accepted(v, ref.v.v, ref.v.e)
            p, m, v = P.restate_adam(inp, t0, 'count_after_increment')
            assert not accepted(p, ref.p.v, ref.p.e) and accepted(m, ref.m.v, ref.m.e)
