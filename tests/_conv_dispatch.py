"""tdg_conv2d_dispatch from Python, and the rows of tests/golden/conv_dispatch.json (no GPU, no torch).

The table was recorded from the library BEFORE the conv dispatch was gathered into choose-then-launch: on a machine
without a GPU its entry points decide, note the kernel and only then fail to launch.  Its layout (indices into the
tables of the same file keep it small):

    descs    [[n, h, w, c, cs, oh, ow, k, ks, kh, kw, stride, pad_t, pad_l, dtype], ...]      TdgConvDesc
    epis     [null | {accumulate, mask, splitk_ws_bytes, col_partial_bytes}, ...]              what the choice reads of TdgEpilogue
    envs     [{TDG_*: value}, ...]                                                              the switches set for the row
    results  [kernel name | status, ...]                                                        a status: the argument checks refused
    rows     [[desc, n_images, form, epi, n_first, env, result], ...]                           form: TDG_FORM_*; n_first: bwd_filter2

Run as a script (`python _conv_dispatch.py i j ...`) it answers the rows with those indices under the environment it
was started with and prints a JSON list: the read-once switches need a process of their own per setting.
"""
import ctypes as C
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = os.path.join(ROOT, 'tests', 'golden', 'conv_dispatch.json')
FORMS = {'fwd': 0, 'bwd_data': 1, 'bwd_filter': 2}
# read once per process (ConvSwitches in 3dgan_amd/csrc/tdg_igemm.hip): a row that sets one is answered by a fresh process
ONCE = {'TDG_KSLICE', 'TDG_TAPORDER', 'TDG_DMA_BM', 'TDG_RING', 'TDG_COL2IM', 'TDG_C2I_MAXCOL', 'TDG_C2I_KB', 'TDG_FUSE', 'TDG_THIN',
        'TDG_CONVN1', 'TDG_WG256', 'TDG_WSPLIT', 'TDG_WDMA_MINKK'}
PER_CALL = {'TDG_DMA', 'TDG_DMA_NW', 'TDG_KSPLIT', 'TDG_PATCH', 'TDG_PATCH_BM', 'TDG_PATCH128', 'TDG_BP', 'TDG_BLOCKPATCH', 'TDG_FWD_N112',
            'TDG_WS128', 'TDG_EFF', 'TDG_WDMA', 'TDG_WDMA_SLOWA', 'TDG_WPATCH', 'TDG_WPATCH_NW'}
_DUMMY = 1 << 16          # stands for a device pointer: the query reads only whether it is NULL


def lib_module():
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    return importlib.import_module('3dgan_amd._lib')


def flags_of(epi):
    """The row form of a ctypes Epilogue (or None)."""
    if epi is None:
        return None
    return {'accumulate': int(epi.accumulate), 'mask': int(epi.mask_mode != 0), 'splitk_ws_bytes': int(epi.splitk_ws_bytes) if epi.splitk_ws else 0,
            'col_partial_bytes': int(epi.col_partial_bytes) if epi.col_partial and epi.col_mode and epi.col_nblk_out else 0}


def epilogue_of(L, flags):
    """(Epilogue | None, keep-alive) with dummy pointers wherever the row says a pointer is set."""
    if flags is None:
        return None, None
    e = L.Epilogue()
    e.accumulate = flags['accumulate']
    if flags['mask']:
        e.mask_mode, e.mask_src = L.MASK_LRELU, _DUMMY
    if flags['splitk_ws_bytes']:
        e.splitk_ws, e.splitk_ws_bytes = _DUMMY, flags['splitk_ws_bytes']
    nblk = C.c_int32(-1)
    if flags['col_partial_bytes']:
        e.col_partial, e.col_partial_bytes, e.col_mode = _DUMMY, flags['col_partial_bytes'], L.COL_SUM
        e.col_nblk_out = C.pointer(nblk)
    return e, nblk


def ask(desc, n_images, form, epi, n_first=0):
    """tdg_conv2d_dispatch: the kernel name, or the status when the argument checks refuse.  `desc`, `epi`: ctypes structures."""
    L = lib_module()
    lib = L.load()
    name = C.create_string_buffer(96)
    rc = lib.tdg_conv2d_dispatch(C.byref(desc), n_images, FORMS.get(form, form), C.byref(epi) if epi is not None else None, n_first, name, len(name))
    return name.value.decode() if rc == 0 else rc


def ask_row(table, row):
    L = lib_module()
    d, n_images, form, e, n_first, _, _ = row
    epi, keep = epilogue_of(L, table['epis'][e])
    got = ask(L.ConvDesc(*table['descs'][d]), n_images, form, epi, n_first)
    if keep is not None and epi.col_nblk_out:
        assert keep.value == -1, 'the query wrote through col_nblk_out'
    return got


def load_table():
    with open(TABLE) as f:
        return json.load(f)


if __name__ == '__main__':
    t = load_table()
    print(json.dumps([ask_row(t, t['rows'][int(i)]) for i in sys.argv[1:]]))
