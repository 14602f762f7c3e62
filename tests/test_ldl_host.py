"""LDL, host side (no GPU): the three entry points of csrc/ldl.hip are declared and exported, they refuse what
the kernels do not cover with SR_EINVAL and a message before any launch, CPU tensors are refused, and the
reference's LDL option file (stored unchanged under tests/golden/reference_options/) parses."""
import ctypes
import os

import pytest
import torch

from basicsr4rs_amd import _lib

REF = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'reference_options')
D = ctypes.c_void_p(16)


def _fwd(lib, N=1, C=3, H=4, W=4, ksize=7, l1=1, red=_lib.REDUCE_MEAN, dt=(0, 0, 0), out=D, gt=D, ema=D, w=None, planes=D,
         stats=D, loss=D, ws=D, ws_bytes=None):
    ws_bytes = lib.sr_ldl_map_workspace(N, max(H, 1), max(W, 1)) if ws_bytes is None else ws_bytes
    return lib.sr_ldl_map_fwd(dt[0], dt[1], dt[2], out, gt, ema, N, C, H, W, ksize, l1, red, 1.0, w, planes, stats, loss, ws,
                              ws_bytes, None)


def _bwd(lib, N=1, C=3, H=4, W=4, ksize=7, red=_lib.REDUCE_MEAN, dt=(0, 0), out=D, gt=D, planes=D, stats=D, dW=None,
         up=None, dout=D, ws=D, ws_bytes=None):
    ws_bytes = lib.sr_ldl_map_workspace(N, max(H, 1), max(W, 1)) if ws_bytes is None else ws_bytes
    return lib.sr_ldl_map_bwd(dt[0], dt[1], out, gt, planes, stats, dW, up, N, C, H, W, ksize, red, 1.0, dout, ws, ws_bytes,
                              None)


def test_symbols_declared_and_exported():
    lib = _lib.load()
    for name, nargs in (('sr_ldl_map_workspace', 3), ('sr_ldl_map_fwd', 21), ('sr_ldl_map_bwd', 19)):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
        assert len(_lib.SIGNATURES[name][1]) == nargs
    assert _lib.SIGNATURES['sr_ldl_map_workspace'][0] is ctypes.c_size_t
    # one (count, mean, M2, S) partial per 64 x 16 tile and image, and the T_n partials of the general backward
    assert lib.sr_ldl_map_workspace(4, 256, 256) >= 4 * 4 * 16 * 16
    assert lib.sr_ldl_map_workspace(2, 70, 135) >= 2 * 3 * 5 * 16


def test_refusals_launch_nothing():
    lib = _lib.load()

    def refused(rc, text):
        assert rc == -1 and text in lib.sr_last_error(), (rc, lib.sr_last_error())

    for call in (_fwd, _bwd):
        refused(call(lib, H=3), b'at least 4')
        refused(call(lib, W=3), b'at least 4')
        refused(call(lib, ksize=5), b'ksize 7 only')
        refused(call(lib, C=0), b'C positive')
        refused(call(lib, N=0), b'N must be')
        refused(call(lib, N=8, C=4, H=8192, W=8192), b'below 2^31')
        refused(call(lib, out=None), b'null pointer')
        refused(call(lib, gt=None), b'null pointer')
        refused(call(lib, planes=None), b'null pointer')
        refused(call(lib, stats=None), b'null pointer')
    refused(_fwd(lib, ema=None), b'null pointer')
    refused(_fwd(lib, ws=None), b'null pointer')
    refused(_fwd(lib, loss=None), b'needs loss')                      # the L1 term without a loss scalar
    refused(_fwd(lib, l1=0, w=None), b'the bare map needs w')
    refused(_fwd(lib, red=_lib.REDUCE_NONE), b"'mean' / 'sum'")
    refused(_fwd(lib, dt=(0, 1, 0)), b"out's dtype")                  # fp32 out with a bf16 gt
    refused(_fwd(lib, dt=(1, 1, 2)), b"out's dtype")
    refused(_fwd(lib, N=2, H=70, W=135, ws_bytes=lib.sr_ldl_map_workspace(2, 70, 135) - 1), b'workspace too small')
    refused(_fwd(lib, out=ctypes.c_void_p(18)), b'element-aligned')
    refused(_bwd(lib, dout=None), b'null pointer')
    refused(_bwd(lib, dW=D, ws=None), b'null pointer')
    refused(_bwd(lib, dW=D, N=2, H=70, W=135, ws_bytes=lib.sr_ldl_map_workspace(2, 70, 135) - 1), b'workspace too small')
    refused(_bwd(lib, red=_lib.REDUCE_NONE), b"'mean' / 'sum'")
    refused(_bwd(lib, dt=(0, 1)), b"out's dtype")
    refused(_bwd(lib, dout=ctypes.c_void_p(18)), b'element-aligned')


def test_cpu_tensors_raise():
    from basicsr4rs_amd.losses.loss_util import get_refined_artifact_map, ldl_l1_term
    a, b, c = torch.rand(1, 3, 8, 8), torch.rand(1, 3, 8, 8), torch.rand(1, 3, 8, 8)
    for ksize in (7, 5):
        with pytest.raises(NotImplementedError, match='run on the MI355X device'):
            get_refined_artifact_map(a, b, c, ksize)
    with pytest.raises(NotImplementedError, match='run on the MI355X device'):
        ldl_l1_term(a, b, c)


def test_ldl_option_file_parses(tmp_path):
    import basicsr4rs_amd.archs  # noqa: F401
    import basicsr4rs_amd.data  # noqa: F401
    import basicsr4rs_amd.losses  # noqa: F401
    import basicsr4rs_amd.models  # noqa: F401
    from basicsr4rs_amd.utils.options import parse_options
    from basicsr4rs_amd.utils.registry import ARCH_REGISTRY, DATASET_REGISTRY, LOSS_REGISTRY, MODEL_REGISTRY
    opt, _ = parse_options(str(tmp_path), is_train=True,
                           argv=['-opt', os.path.join(REF, 'train', 'LDL', 'train_LDL_Real_x4.yml')])
    assert opt['model_type'] == 'RealESRGANModel' and opt['model_type'] in MODEL_REGISTRY
    assert opt['network_g']['type'] in ARCH_REGISTRY and opt['network_d']['type'] == 'UNetDiscriminatorSN'
    assert opt['datasets']['train']['type'] in DATASET_REGISTRY
    tr = opt['train']
    assert tr['ldl_opt'] == dict(type='L1Loss', loss_weight=1.0, reduction='mean') and tr['ldl_opt']['type'] in LOSS_REGISTRY
    assert tr['ema_decay'] == 0.999 and opt['gt_size'] == 256
    assert opt['datasets']['train']['batch_size_per_gpu'] == 4
