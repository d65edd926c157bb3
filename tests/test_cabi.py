"""The C-ABI library loads without a GPU and exports exactly what include/tdg.h declares."""
import os
import re
import subprocess

from conftest import pkg, ROOT


def declared_symbols():
    text = open(os.path.join(ROOT, 'include', 'tdg.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    return set(re.findall(r'\b(tdg_[a-z0-9_]+)\s*\(', text))


def test_header_python_and_library_agree():
    L = pkg('_lib')
    lib = L.load()                                   # raises if the .so is missing: there is no CPU fallback
    decl = declared_symbols()
    assert decl == set(L.SIGNATURES), decl ^ set(L.SIGNATURES)
    out = subprocess.check_output(['nm', '-D', '--defined-only', L.LIB_PATH]).decode()
    exported = set(re.findall(r' T (tdg_[a-z0-9_]+)', out))
    assert decl <= exported, decl - exported
    assert lib.tdg_version() >= 100


def test_argument_errors_are_reported_not_thrown():
    """Status + tdg_last_error(), never an exception across the boundary (no GPU work is enqueued)."""
    import ctypes as C
    L = pkg('_lib')
    lib = L.load()
    d = L.ConvDesc(1, 8, 8, 4, 4, 4, 4, 8, 8, 5, 5, 3, 1, 1, 0)          # stride 3: unsupported
    assert lib.tdg_packed_filter_fwd_bytes(C.byref(d)) == 0
    assert b'stride' in lib.tdg_last_error()
    rc = lib.tdg_adam_step(None, None, None, None, 16, 0.1, 0.9, 0.999, 1e-8, 1.0, None)
    assert rc == -1 and b'tdg_adam_step' in lib.tdg_last_error()
    d = L.ConvDesc(1, 8, 8, 4, 2, 4, 4, 8, 8, 5, 5, 2, 1, 1, 0)          # channel stride < channels
    assert lib.tdg_packed_filter_bwd_bytes(C.byref(d)) == 0
    # sizes for a valid descriptor: K = 25*8 = 200 f32 -> padded to 224 per row of the 16 output channels
    d = L.ConvDesc(2, 8, 8, 8, 8, 4, 4, 16, 16, 5, 5, 2, 1, 1, 0)
    assert lib.tdg_packed_filter_fwd_bytes(C.byref(d)) == 16 * 224 * 4
    assert lib.tdg_conv2d_bwd_filter_workspace_bytes(C.byref(d), 2) >= 25 * 8 * 16 * 4


def test_sizes_of_each_conv_form():
    """Packed filter and filter-gradient workspace sizes of one descriptor per form (values of the implementation before
    the sizing, packing and launch code shared one plan per direction)."""
    import ctypes as C
    L = pkg('_lib')
    lib = L.load()
    cases = [  # (n, h, w, c, cs, oh, ow, k, ks, kh, kw, stride, pad_t, pad_l, dtype): fwd, bwd, workspace (n, n // 2 images)
        ((64, 64, 64, 3, 4, 32, 32, 200, 200, 5, 5, 2, 1, 1, 1), (46592, 64768, 15360000, 7680000)),           # thin / fused
        ((64, 8, 8, 400, 400, 4, 4, 800, 800, 5, 5, 2, 1, 1, 1), (16076800, 16025600, 96000000, 64000000)),   # 5-chunk K slices
        ((16, 64, 64, 2, 2, 32, 32, 64, 64, 4, 4, 2, 1, 1, 1), (8192, 4096, 524288, 262144)),                 # scalar gather / col2im
        ((16, 64, 64, 3, 4, 32, 32, 16, 16, 4, 4, 2, 1, 1, 1), (2048, 3072, 196608, 98304)),                  # col2im
        ((16, 32, 32, 64, 64, 16, 16, 128, 128, 4, 4, 2, 1, 1, 1), (262144, 262144, 8388608, 4194304)),       # parity classes
        ((16, 32, 32, 50, 50, 16, 16, 100, 100, 5, 5, 2, 2, 2, 1), (256000, 268800, 8000000, 4000000)),       # compact strides
        ((2, 8, 8, 8, 8, 4, 4, 16, 16, 5, 5, 2, 1, 1, 0), (14336, 13312, 12800, 12800)),                       # f32
    ]
    for t, want in cases:
        d = L.ConvDesc(*t)
        got = (lib.tdg_packed_filter_fwd_bytes(C.byref(d)), lib.tdg_packed_filter_bwd_bytes(C.byref(d)),
               lib.tdg_conv2d_bwd_filter_workspace_bytes(C.byref(d), t[0]),
               lib.tdg_conv2d_bwd_filter_workspace_bytes(C.byref(d), t[0] // 2))
        assert got == want, (t, got, want)


def test_missing_library_fails_loudly(monkeypatch):
    L = pkg('_lib')
    import pytest
    monkeypatch.setattr(L, '_lib', None)
    monkeypatch.setattr(L, 'LIB_PATH', '/nonexistent/lib3dgan_hip.so')
    with pytest.raises(L.TdgError):
        L.load()
