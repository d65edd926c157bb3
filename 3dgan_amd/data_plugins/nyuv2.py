"""NYU Depth v2 RGB -> depth pairs (hem/data/nyuv2.py), the input of `--model pix2pix` (examples/pix2pix.config).

Records (`nyuv2.train.tfrecords`, written by hem/data/nyuv2.py:121-146): `image` = PNG bytes of the 8-bit RGB frame,
`depth` = PNG bytes of the 16-bit depth frame, plus width / height / channels / filenames.  Parsing as in
`parse_tfrecord` (:148-246): decode_png; optional `--resize W H` (TF-1.x bilinear) or `--random_crop H W` (one crop
window per draw, the same for image and depth, :206-208); image / 255, depth / 65535; pairs whose depth crop contains an
exact 0 or 1 are dropped (`ignore_incomplete_depthmaps`, :258-262, which looks at y alone).  Output per batch, in the
reference's order (:244-251), all NHWC f32 on the device:

    (x [B,h,w,3], y [B,h,w,1] [, x_loc, y_loc] [, mean_vec] [, x_full, y_full])

  x_loc, y_loc [B,ch,cw,1]   `--random_crop` with `--include_location` (:157-162,188-200): the ramps x_loc[r, c] = c / (W - 1),
                             y_loc[r, c] = r / (H - 1) of the frame's own H x W (the reference hard-codes 427 and 561), resized
                             like the pair under `--resize`, cut by the pair's window.
  mean_vec [B,h,w,1]         `--normalize` (:220-223): every pixel the mean of that image's final [0, 1] depth.  The depth itself
                             is unchanged (the reference's subtraction is commented out).
  x_full [B,A,B',3], y_full [B,A,B',1]   `--include_originals A B'` (:167-177): the whole frame resized (TF-1.x bilinear) to A rows
                             by B' columns -- tf.image.resize_images takes (height, width) whatever the flag's help says --
                             then / 255 and / 65535.  Frames are static: all N are resized once, when the source is built.
"""
import os

import numpy as np
import torch

from .DataPlugin import DataPlugin, find_file, dataset_dirs, write_cache_atomically
from ._common import resize_bilinear_tf1
from .. import tfrecord, png

_dataset_files = {'train': 'nyuv2.train.tfrecords', 'validate': 'nyuv2.validate.tfrecords', 'test': 'nyuv2.test.tfrecords'}


class PairSource:
    """Device-resident decoded frames; every next_batch() draws B frames (shuffled epoch order, per-replica shard), one
    random crop window per frame, and re-draws windows whose depth crop holds an exact 0 or 1."""

    def __init__(self, rgb_u8, depth_u16, batch_size, device, crop, resize, seed, rank, world, location=False, normalize=False,
                 originals=None):
        self.rgb = torch.from_numpy(rgb_u8[rank::world] if world > 1 else rgb_u8).to(device)            # [N, H, W, 3] uint8
        self.depth = torch.from_numpy((depth_u16[rank::world] if world > 1 else depth_u16).astype(np.int32)).to(device)
        self.B, self.device, self.crop, self.resize = batch_size, device, crop, resize
        self.gen = torch.Generator(device='cpu').manual_seed(int(seed) + 7919 * rank)
        self.n = self.rgb.shape[0]
        self.barren_passes = 8                       # give up after this many passes over the shard without ONE valid crop
        if not crop:
            # without a random window a frame's verdict never changes: decide once, then draw only frames that pass
            # (the reference's filter is unbounded, hem/data/nyuv2.py:258-266; re-testing them every epoch is not)
            keep = []
            for i0 in range(0, self.n, 64):
                idx = torch.arange(i0, min(i0 + 64, self.n))
                keep.append(idx[self._complete(self._make(idx)[1]).cpu()])
            keep = torch.cat(keep) if keep else torch.zeros(0, dtype=torch.long)
            if keep.numel() == 0:
                raise RuntimeError('nyuv2: every one of the %d depth maps has sensor gaps (an exact 0 or 1)' % self.n)
            self.rgb, self.depth = self.rgb[keep.to(device)], self.depth[keep.to(device)]
            self.n = int(keep.numel())
        self.perm, self.i = torch.randperm(self.n, generator=self.gen), 0
        # the three optional outputs; none of them draws from the generator
        self.normalize = bool(normalize)
        self.loc = self._ramps() if (location and crop) else None                # (:245: only with a random crop)
        self.full = self._originals(*originals) if originals else None

    def _ramps(self):
        """[2, h, w, 1]: x_loc then y_loc of the (resized) frame."""
        H, W = int(self.rgb.shape[1]), int(self.rgb.shape[2])
        cols = (torch.arange(W, dtype=torch.float64) / max(W - 1, 1)).float()
        rows = (torch.arange(H, dtype=torch.float64) / max(H - 1, 1)).float()
        loc = torch.stack([cols[None, :].expand(H, W), rows[:, None].expand(H, W)])[..., None].to(self.device)
        if self.resize:
            w, h = self.resize
            loc = resize_bilinear_tf1(loc, h, w)
        return loc.contiguous()

    def _originals(self, out_h, out_w):
        """(x_full [N, out_h, out_w, 3], y_full [N, out_h, out_w, 1]) of every frame of the shard, 64 frames at a time."""
        xs, ys = [], []
        for i0 in range(0, self.n, 64):
            xs.append(resize_bilinear_tf1(self.rgb[i0:i0 + 64].float(), out_h, out_w) / 255.0)
            ys.append(resize_bilinear_tf1(self.depth[i0:i0 + 64].float()[..., None], out_h, out_w) / 65535.0)
        return torch.cat(xs).contiguous(), torch.cat(ys).contiguous()

    def _indices(self, k):
        out = []
        while len(out) < k:
            if self.i >= self.n:
                self.perm, self.i = torch.randperm(self.n, generator=self.gen), 0
            take = min(k - len(out), self.n - self.i)
            out.append(self.perm[self.i:self.i + take])
            self.i += take
        return torch.cat(out)

    def _make(self, idx):
        """(x, y, window) of the frames `idx`; window = (rows [k, ch], cols [k, cw]) of the drawn crop, or None."""
        win = None
        rgb, depth = self.rgb[idx.to(self.device)], self.depth[idx.to(self.device)]
        x = rgb.float()
        y = depth.float()[..., None]
        if self.resize:
            w, h = self.resize
            x, y = resize_bilinear_tf1(x, h, w), resize_bilinear_tf1(y, h, w)
        if self.crop:
            ch, cw = self.crop
            H, W = x.shape[1], x.shape[2]
            top = torch.randint(0, H - ch + 1, (len(idx),), generator=self.gen).to(self.device)
            left = torch.randint(0, W - cw + 1, (len(idx),), generator=self.gen).to(self.device)
            rows = (top[:, None] + torch.arange(ch, device=self.device)[None])                  # [k, ch]
            cols = (left[:, None] + torch.arange(cw, device=self.device)[None])                 # [k, cw]
            bi = torch.arange(len(idx), device=self.device)[:, None, None]
            x = x[bi, rows[:, :, None], cols[:, None, :]]
            y = y[bi, rows[:, :, None], cols[:, None, :]]
            win = (rows, cols)
        return x / 255.0, y / 65535.0, win

    def _extras(self, idx, y, win):
        """The optional outputs of the pairs (`idx`, y, window), in the reference's order."""
        out = []
        if self.loc is not None:
            rows, cols = win
            out += [self.loc[k][rows[:, :, None], cols[:, None, :]] for k in (0, 1)]
        if self.normalize:
            out.append(y.mean(dim=(1, 2, 3), keepdim=True).expand_as(y))
        if self.full is not None:
            i = idx.to(self.device)
            out += [self.full[0][i], self.full[1][i]]
        return out

    @staticmethod
    def _complete(y):
        flat = y.reshape(y.shape[0], -1)
        return ~((flat == 0).any(1) | (flat == 1).any(1))                     # hem/data/nyuv2.py:258-262

    def next_batch(self):
        """Frames are redrawn until B crops pass the filter, however sparse the valid ones are (the reference's filter is
        unbounded); the only failure is NO progress: `barren_passes` whole passes over the shard without a single valid crop."""
        xs, ys, es, need, barren = [], [], [], self.B, 0
        while need > 0:
            idx = self._indices(need)
            x, y, win = self._make(idx)
            ok = self._complete(y) if self.crop else torch.ones(y.shape[0], dtype=torch.bool, device=y.device)
            if ok.any():
                xs.append(x[ok])
                ys.append(y[ok])
                es.append([e[ok] for e in self._extras(idx, y, win)])
                need -= int(ok.sum())
                barren = 0
            else:
                barren += int(y.shape[0])
                if barren >= self.barren_passes * max(self.n, 1):
                    raise RuntimeError('nyuv2: no depth crop without sensor gaps in %d passes over %d frames' % (self.barren_passes, self.n))
        return tuple(torch.cat(t)[:self.B].contiguous() for t in [xs, ys] + [list(e) for e in zip(*es)])


class NYUv2Dataset(DataPlugin):
    name = 'nyuv2'

    @staticmethod
    def arguments():
        """hem/data/nyuv2.py:40-78."""
        return {
            '--resize': {'type': int, 'nargs': 2, 'help': 'Resize input images to size w x h.'},
            '--random_crop': {'type': int, 'nargs': 2, 'help': 'Randomly crop the input images to size h x w.'},
            '--include_location': {'action': 'store_true', 'default': False,
                                   'help': 'With --random_crop: also emit the x / y location ramps of each crop window.'},
            '--skip_invalid': {'action': 'store_true', 'default': False,
                               'help': 'Parsed but unused by the reference; depth maps with gaps are always dropped.'},
            '--normalize': {'action': 'store_true', 'default': False,
                            'help': 'Also emit a channel holding the mean of each depth image (the depth itself is unchanged).'},
            '--include_originals': {'type': int, 'nargs': 2,
                                    'help': 'Also emit the whole frames resized to h x w (rows, then columns), image and depth.'},
        }

    @staticmethod
    def check_prepared_datasets(storage_dir):
        return DataPlugin.check_files(storage_dir, list(_dataset_files.values()))

    @staticmethod
    def load(args, split='train'):
        cache = os.path.join(args.cache_dir, 'nyuv2.%s.npz' % split) if getattr(args, 'cache_dir', None) else None
        if cache and os.path.exists(cache):
            z = np.load(cache)
            return z['rgb'], z['depth']
        tfr = find_file(args, [_dataset_files[split]])
        if not tfr:
            raise FileNotFoundError('no %s under %s; use --dataset synthetic' % (_dataset_files[split], dataset_dirs(args)))
        rgb, depth = [], []
        for rec in tfrecord.read_records(tfr):
            ex = tfrecord.parse_example(rec)
            rgb.append(png.decode(ex['image'], channels=3))                 # hem/data/nyuv2.py:152
            d = png.decode(ex['depth'], channels=1)                         # :153 (dtype uint16)
            depth.append(d[..., 0].astype(np.uint16) if d.dtype != np.uint16 else d[..., 0])
        rgb, depth = np.stack(rgb), np.stack(depth)
        if cache:
            write_cache_atomically(cache, lambda f: np.savez(f, rgb=rgb, depth=depth))
        return rgb, depth

    @staticmethod
    def get_source(args, sess, split='train'):
        """`split`: which records feed the source (paper_metrics.py opens `validate` too)."""
        rgb, depth = NYUv2Dataset.load(args, split)
        crop = tuple(args.random_crop) if getattr(args, 'random_crop', None) else None
        seed = args.seed if isinstance(getattr(args, 'seed', None), int) else 0
        originals = tuple(args.include_originals) if getattr(args, 'include_originals', None) else None
        src = PairSource(rgb, depth, args.batch_size, sess.device, crop, getattr(args, 'resize', None), seed, sess.rank,
                         sess.world_size, location=bool(getattr(args, 'include_location', False)),
                         normalize=bool(getattr(args, 'normalize', False)), originals=originals)
        h, w = crop if crop else ((args.resize[1], args.resize[0]) if getattr(args, 'resize', None) else rgb.shape[1:3])
        return src, rgb.shape[0], (h, w, 3)
