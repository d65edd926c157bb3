"""Digests of the variables after one train() of two models that other work must not disturb: paper_cgan
--model_version mean_adjusted (B = 4, f32, eager) and pix2pix --noise input latent end (B = 1, f32, eager).  Per variable the
SHA-256 of its float32 bytes and its float64 sum.  `python tools/regression_digest.py OUT.npz` writes them;
tests/test_gpu_paper_sampler.py compares the tree it runs in against tests/golden/regression_digests.npz.  `--sampler OUT.npz`
writes the same for the plugins of models/sampler/ (sampler_digests(); tests/golden/sampler_parent_digests.npz, compared by
tests/test_gpu_paper_standalone.py).  `--depth OUT.npz` writes depth_digests(): the outputs of the depth models' reduction,
whole-frame and evaluation kernels and of infer_full / evaluate / metrics / sample_full, per named output
(tests/golden/depth_parent_digests.npz, compared by tests/test_gpu_depth_parent_digests.py)."""
import hashlib
import importlib
import os
import sys
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402


class Pairs:
    def __init__(self, B, side, n, seed, device):
        g = torch.Generator().manual_seed(seed)
        self.x = [torch.rand(B, side, side, 3, generator=g).to(device) for _ in range(n)]
        self.y = [(torch.rand(B, side, side, 1, generator=g) * 0.98 + 0.01).to(device) for _ in range(n)]
        self.i = 0

    def next_batch(self):
        k = self.i % len(self.x)
        self.i += 1
        return self.x[k], self.y[k]


def models(device):
    rt = importlib.import_module('3dgan_amd.runtime')
    sess = rt.Session(device=device, dtype=0, seed=0, rank=0, world_size=1)
    args = SimpleNamespace(batch_size=4, n_gpus=1, model_version='mean_adjusted', training_version='gan', seed=0, use_graphs=False,
                           g_lr=2e-5, d_lr=1e-5, g_beta1=0.5, d_beta1=0.8, g_beta2=0.99, d_beta2=0.995)
    yield 'paper_cgan', importlib.import_module('3dgan_amd.models.paper.paper_cgan').paper_cgan(Pairs(4, 65, 2, 0, device), args, sess)
    sess = rt.Session(device=device, dtype=0, seed=0, rank=0, world_size=1)
    args = SimpleNamespace(model='pix2pix', batch_size=1, n_gpus=1, optimizer='adam', lr=1e-4, beta1=0.5, beta2=0.999, decay=0.9,
                           momentum=0.01, centered=False, n_disc_train=1, add_l1=True, batch_norm_gen=False, batch_norm_disc=False,
                           dropout=0, noise=['input', 'latent', 'end'], seed=0, use_graphs=False)
    yield 'pix2pix', importlib.import_module('3dgan_amd.models.pix2pix').pix2pix(Pairs(1, 256, 2, 1, device), args, sess)


def sampler_models(device):
    """The plugins of models/sampler/, which run on the skip U-Net executor's noise windows: paper_sampler at e1 and d4 with
    encoder batch norm and at x without, and paper_noise; each at B = 4, f32, seed 0, eager."""
    rt = importlib.import_module('3dgan_amd.runtime')
    hp = dict(g_lr=2e-5, d_lr=1e-5, g_beta1=0.5, d_beta1=0.8, g_beta2=0.99, d_beta2=0.995)
    for tag, model, node, bn in (('paper_sampler_e1_bn', 'paper_sampler', 'e1', True), ('paper_sampler_d4_bn', 'paper_sampler', 'd4', True),
                                 ('paper_sampler_x', 'paper_sampler', 'x', False), ('paper_noise', 'paper_noise', 'x', False)):
        sess = rt.Session(device=device, dtype=0, seed=0, rank=0, world_size=1)
        if model == 'paper_noise':
            args = SimpleNamespace(batch_size=4, n_gpus=1, model_version='baseline', seed=0, use_graphs=False, **hp)
        else:
            args = SimpleNamespace(batch_size=4, n_gpus=1, noise_layer=node, e_bn='false', e_bn_off=not bn, seed=0, use_graphs=False, **hp)
        cls = getattr(importlib.import_module('3dgan_amd.models.sampler.' + model), model)
        yield tag, cls(Pairs(4, 65, 2, 0, device), args, sess)


def sampler_digests(device=None):
    """digests() of sampler_models(): tests/golden/sampler_parent_digests.npz (`python tools/regression_digest.py --sampler OUT.npz`)."""
    device = device or torch.device('cuda:0')
    out = {}
    for name, m in sampler_models(device):
        m.train(None, None, None)
        torch.cuda.synchronize()
        for k, v in sorted(m.variables().items()):
            a = np.ascontiguousarray(v, dtype=np.float32)
            out[name + '/' + k] = (hashlib.sha256(a.tobytes()).hexdigest(), float(a.astype(np.float64).sum()))
    return out


def digests(device=None):
    """{'<model>/<variable>': (sha256 hex, float64 sum)} after one train() of each model."""
    device = device or torch.device('cuda:0')
    out = {}
    for name, m in models(device):
        m.train(None, None, None)
        torch.cuda.synchronize()
        for k, v in sorted(m.variables().items()):
            a = np.ascontiguousarray(v, dtype=np.float32)
            out[name + '/' + k] = (hashlib.sha256(a.tobytes()).hexdigest(), float(a.astype(np.float64).sum()))
    return out


# ------------------------------------------------------------------------------------------------ depth models
HW = 29 * 29
FRAME = (113, 107, 6)            # H, W, stride: (113 - 93) // 6 = 3 windows down, (107 - 93) // 6 = 2 across, 6 windows
SLICED = (1, 7, 8, 9, 17)        # images / draws against the 8 slices of a moments block: fewer, equal, one more, two rounds + 1


def _put(out, name, *values):
    """Digest of the raw bytes of `values` (device tensors, arrays or scalars) in order, whatever their dtypes."""
    parts = [np.ascontiguousarray(v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)) for v in values]
    with np.errstate(all='ignore'):
        total = float(sum(p.astype(np.float64).sum() for p in parts))
    assert name not in out, name
    out[name] = (hashlib.sha256(b''.join(p.tobytes() for p in parts)).hexdigest(), total)


def depth_frame():
    H, W, _ = FRAME
    rng = np.random.default_rng(31)
    return rng.random((H, W, 3), dtype=np.float32), (rng.random((H, W), dtype=np.float32) * 0.98 + 0.01).astype(np.float32)


def depth_kernel_digests(device, out):
    """The entry points of the depth .hip files on seeded f32 inputs, hw = 841."""
    L = importlib.import_module('3dgan_amd._lib')
    K = importlib.import_module('3dgan_amd.kernels')
    lib = L.load()
    keep = []

    def dev(a, dtype=torch.float32):
        keep.append(torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device=device))     # alive until the function returns
        return keep[-1]

    def zeros(*shape, dtype=torch.float32, fill=0):
        return dev(np.full(shape, fill), dtype)

    p = lambda t: K.ptr(t)
    f = np.float32

    def batch(n, seed):
        """The crop in [0.1, 10], g, a prediction with negative entries, per-image offsets, a [0, 1] image."""
        rng = np.random.default_rng([seed, n])
        y = rng.uniform(0.1, 10, (n, HW)).astype(f)
        g = (y * rng.uniform(0.6, 1.6, (n, HW))).astype(f) - f(1.0)
        off = rng.uniform(0.5, 1.5, n).astype(f)
        return y, g, (g + off[:, None]).astype(f), off, rng.uniform(0.05, 0.95, HW).astype(f)

    def eval_buffers():
        return (zeros(lib.tdg_cgan_eval_acc_bytes(HW) // 8, dtype=torch.float64), zeros(3, 4, dtype=torch.int64),
                zeros(lib.tdg_cgan_eval_workspace_bytes(), dtype=torch.uint8), zeros(3, 12, dtype=torch.float64), zeros(HW), zeros(HW))

    # ---- tdg_cgan_eval.hip, tdg_cgan_metrics (tdg_cgan.hip)
    for n in SLICED:
        acc, counts, ws, scalars, mean, var = eval_buffers()
        for k in range(2):                                                      # two batches: the second adds to the first
            L.call('tdg_cgan_eval_moments', p(dev(batch(n, 1 + k)[0])), n, HW, p(acc), K.stream())
        L.call('tdg_cgan_eval_finish', p(acc), p(counts), HW, 10.0, p(scalars), p(mean), p(var), K.stream())
        _put(out, 'kernel/eval_moments/n%d' % n, acc, mean, var)
    n = 6
    acc, counts, ws, scalars, mean, var = eval_buffers()
    for k in range(2):
        y, g, pred, off, img = batch(n, 3 + k)
        L.call('tdg_cgan_eval_batch', p(dev(y)), p(dev(pred)), p(dev(off)), p(dev(img)), 10.0, n, HW, 7, p(counts), p(acc), p(ws),
               ws.numel(), K.stream())
    L.call('tdg_cgan_eval_finish', p(acc), p(counts), HW, 10.0, p(scalars), None, None, K.stream())
    _put(out, 'kernel/eval_batch', acc[:27], counts, scalars)
    mcounts, mout = zeros(4, dtype=torch.int64), zeros(8)
    mws = zeros(lib.tdg_cgan_metrics_workspace_bytes(), dtype=torch.uint8)
    for tag, pr, of in (('pred_offset', g, off), ('offset', None, off)):
        L.call('tdg_cgan_metrics', p(dev(y)), p(dev(pr) if pr is not None else None), p(dev(of)), n, HW, p(mcounts), p(mout), p(mws),
               mws.numel(), K.stream())
        _put(out, 'kernel/metrics/' + tag, mout, mcounts)

    # ---- tdg_cgan_sampler.hip
    for n in SLICED:
        y, g, pred, off, img = batch(n, 5)
        sout, mean, var = zeros(6, fill=7.0), zeros(HW, fill=7.0), zeros(HW, fill=7.0)
        ws = zeros(lib.tdg_cgan_sample_stats_workspace_bytes(n, HW), dtype=torch.uint8)
        L.call('tdg_cgan_sample_stats', p(dev(y)), p(dev(g)), p(dev(pred)), p(dev(off)), None, 10.0, n, HW, 10.0, p(sout), p(mean), p(var),
               p(ws), ws.numel(), K.stream())
        _put(out, 'kernel/sample_stats/n%d' % n, sout, mean, var)
    L.call('tdg_cgan_sample_stats', p(dev(y)), None, None, None, p(dev(img)), 10.0, n, HW, 10.0, p(sout), None, None, p(ws), ws.numel(),
           K.stream())
    _put(out, 'kernel/sample_stats/image_form', sout)

    # ---- tdg_cgan.hip: prep, wgan loss
    B = 3
    y65 = np.random.default_rng(7).uniform(0.01, 0.99, (B, 65, 65)).astype(f)
    for version in (0, 1, 2):
        mp2 = version == 2
        depth = K.Act(2 * B, 29, 29, 2 if mp2 else 1, 0, device)
        gx, rx = K.Act(B, 65, 65, 4, 0, device), K.Act(B, 65, 65, 4, 0, device)
        ybar, crop = zeros(B), zeros(B, 29, 29)
        L.call('tdg_cgan_prep', 0, p(dev(y65)), B, version, depth.ptr(0), depth.cs, depth.ptr(B) if mp2 else None, p(ybar), p(crop),
               gx.window(3, 1).ptr(0) if mp2 else None, gx.cs, rx.window(3, 1).ptr(0) if mp2 else None, rx.cs, K.stream())
        _put(out, 'kernel/prep/v%d' % version, depth.buf, ybar, crop, gx.buf, rx.buf)
    rows = 300                                                                  # more rows than the block's 256 threads
    logits = K.Act(2 * rows, 1, 1, 1, 0, device).set(np.random.default_rng(8).uniform(-3, 3, (2 * rows, 1, 1, 1)).astype(f))
    for mode in (0, 1, 2):
        seed, scal = K.Act(2 * rows, 1, 1, 1, 0, device), zeros(4)
        L.call('tdg_cgan_wgan_loss', 0, logits.ptr(), rows, logits.cs, mode, seed.ptr(), p(scal), K.stream())
        _put(out, 'kernel/wgan_loss/mode%d' % mode, scal, seed.buf)

    # ---- tdg_cgan_standalone.hip: three blocks of 1024 elements, the last partial
    n = 3
    y, _, pred, off, _ = batch(n, 9)
    for tag, shift in (('aligned', 0), ('misaligned', 1)):
        yd, pd = zeros(n * HW + 4), zeros(n * HW + 4)
        yd[shift:shift + n * HW].copy_(dev(y).reshape(-1))
        pd[shift:shift + n * HW].copy_(dev(pred).reshape(-1))
        dg, scal = zeros(n * HW, fill=77.0), zeros(2, fill=77.0)
        ws = zeros(max(lib.tdg_cgan_rmse_loss_workspace_bytes(n, HW), 8), dtype=torch.uint8)
        L.call('tdg_cgan_rmse_loss', 0, K.ptr(yd, 4 * shift), K.ptr(pd, 4 * shift), n, HW, p(dg), 1, p(scal), p(ws), ws.numel(), K.stream())
        _put(out, 'kernel/rmse_loss/' + tag, dg, scal)
    win, plane = K.Act(n, 31, 31, 1, 0, device), zeros(n, 31, 31)
    L.call('tdg_cgan_bar_fill', 0, p(dev(off)), n, 31 * 31, win.ptr(0), win.cs, p(plane), K.stream())
    _put(out, 'kernel/bar_fill', win.buf, plane)

    # ---- tdg_cgan_full.hip: gathers, sample store, frame RMSE
    H, W, s = FRAME
    image, depth = depth_frame()
    d_image, d_depth = dev(image), dev(depth)
    canvas = np.random.default_rng(10).uniform(0, 10, (H, W)).astype(f)
    rout, rws = zeros(1, dtype=torch.float64), zeros(256, dtype=torch.float64)
    L.call('tdg_cgan_full_rmse', p(d_depth), p(dev(canvas)), H, W, p(rout), p(rws), 256 * 8, K.stream())
    _put(out, 'kernel/full_rmse', rout)
    for chunk in (0, 1, 2):                                                     # 4 windows a chunk: full, two padded slots, all padding
        x, yy, ch = zeros(4, 65, 65, 3, fill=7.0), zeros(4, 65, 65, 1, fill=7.0), dev([chunk], torch.int32)
        L.call('tdg_cgan_full_gather', p(d_image), p(d_depth), H, W, s, p(ch), 4, p(x), p(yy), K.stream())
        _put(out, 'kernel/full_gather/chunk%d' % chunk, x, yy, ch)
    for rep in (1, 2, 3):
        for B in sorted({b for b in (4, 4 * rep) if b % rep == 0}):            # batch 4 where rep divides it; 4 windows a chunk
            for with_depth in (True, False):
                for chunk in (0, 1, 2):
                    x, yy, ch = zeros(B, 65, 65, 3, fill=7.0), zeros(B, 65, 65, 1, fill=7.0), dev([chunk], torch.int32)
                    L.call('tdg_cgan_full_gather_rep', p(d_image), p(d_depth) if with_depth else None, H, W, s, p(ch), B, rep, p(x), p(yy),
                           K.stream())
                    _put(out, 'kernel/full_gather_rep/rep%d_B%d_%s/chunk%d' % (rep, B, 'depth' if with_depth else 'nodepth', chunk),
                         x, yy, ch)
    for draws in SLICED:
        for groups in (1, 3):
            B = draws * groups
            rng = np.random.default_rng([11, draws, groups])
            yhat = (rng.uniform(1.0, 8.0, (groups, 1, 1)) + 0.3 * rng.standard_normal((groups, draws, HW))).astype(f).reshape(B, HW)
            crop, ybar = rng.uniform(0.1, 9.9, (B, HW)).astype(f), rng.uniform(0.0, 9.0, B).astype(f)
            for with_crop in (True, False):
                nrows = 2 * groups + 2
                sy, sv, sb, se = zeros(nrows, HW, fill=-7.0), zeros(nrows, HW, fill=-7.0), zeros(nrows, fill=-7.0), zeros(nrows, 2, fill=-7.0)
                ch = dev([0], torch.int32)
                for _ in range(3):                                              # chunks 0 and 1 fill the 2 * groups slots, chunk 2 is past them
                    L.call('tdg_cgan_full_sample_store', p(dev(yhat)), p(dev(ybar)), p(dev(crop)) if with_crop else None, B, draws,
                           2 * groups, p(ch), p(sy), p(sv), p(sb), p(se) if with_crop else None, K.stream())
                _put(out, 'kernel/full_sample_store/draws%d_groups%d_%s' % (draws, groups, 'crop' if with_crop else 'nocrop'),
                     sy, sv, sb, se, ch)
    torch.cuda.synchronize()


def _flat(d):
    """A metrics() / evaluate() result as one float64 vector, keys in order."""
    vals = []
    for k in sorted(d):
        v = d[k]
        vals.extend(_flat(v).tolist() if isinstance(v, dict) else np.asarray(v, np.float64).ravel().tolist())
    return np.array(vals, np.float64)


def depth_model_digests(device, out):
    """infer_full / evaluate / metrics of paper_cgan and sample_full of paper_sampler at B = 4, f32, seed 0, graphs at their
    default: each name's first call runs eager, its second captures the body and replays it."""
    rt = importlib.import_module('3dgan_amd.runtime')
    hp = dict(g_lr=2e-5, d_lr=1e-5, g_beta1=0.5, d_beta1=0.8, g_beta2=0.99, d_beta2=0.995)
    H, W, s = FRAME
    image, depth = depth_frame()
    cgan = importlib.import_module('3dgan_amd.models.paper.paper_cgan').paper_cgan
    for version in ('baseline', 'mean_adjusted', 'mean_provided2'):
        sess = rt.Session(device=device, dtype=0, seed=0, rank=0, world_size=1)
        args = SimpleNamespace(batch_size=4, n_gpus=1, model_version=version, training_version='gan', seed=0, **hp)
        m = cgan(Pairs(4, 65, 4, 0, device), args, sess)
        for offset in (18, 17):
            r = m.infer_full(image, depth, stride=s, offset=offset)
            assert r.patches == 6
            _put(out, 'model/paper_cgan_%s/infer_full_offset%d' % (version, offset), r.y_hat, r.g, np.float64(r.rmse))
        _put(out, 'model/paper_cgan_%s/evaluate' % version, _flat(m.evaluate(Pairs(4, 65, 4, 5, device), 2)))
        m.train(None, None, None)
        _put(out, 'model/paper_cgan_%s/metrics' % version, _flat(m.metrics()))
    sampler = importlib.import_module('3dgan_amd.models.sampler.paper_sampler').paper_sampler
    for tag, node, bn, draws in (('bn', 'd3', True, 4), ('bn_off', 'e2', False, 2)):
        sess = rt.Session(device=device, dtype=0, seed=0, rank=0, world_size=1)
        args = SimpleNamespace(batch_size=4, n_gpus=1, noise_layer=node, e_bn='false', e_bn_off=not bn, seed=0, **hp)
        m = sampler(Pairs(4, 65, 2, 0, device), args, sess)
        for with_depth in (True, False) if not bn else (True,):
            r = m.sample_full(image, depth if with_depth else None, stride=s, draws=draws, windows=True)
            assert r.patches == 6
            scalars = [np.float64(v) for v in (r.rmse, r.err_mean, r.err_min)] if with_depth else []
            _put(out, 'model/paper_sampler_%s/sample_full%s' % (tag, '' if with_depth else '_no_depth'), r.y_hat, r.g, r.var,
                 r.window_y_hat, r.window_var, r.window_y_bar, *scalars)
    torch.cuda.synchronize()


def depth_digests(device=None):
    """{'<kernel|model>/<case>': (sha256 hex, float64 sum)} of the depth models' kernels and whole-frame / evaluation paths."""
    device = device or torch.device('cuda:0')
    out = {}
    depth_kernel_digests(device, out)
    depth_model_digests(device, out)
    return out


if __name__ == '__main__':
    mode = sys.argv[1] if sys.argv[1:2] in (['--sampler'], ['--depth']) else None
    if mode:
        del sys.argv[1]
    d = {'--sampler': sampler_digests, '--depth': depth_digests, None: digests}[mode]()
    names = sorted(d)
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
    np.savez(sys.argv[1], names=np.array(names), sha256=np.array([d[k][0] for k in names]), sums=np.array([d[k][1] for k in names]))
    print('wrote %d digests to %s' % (len(names), sys.argv[1]))
