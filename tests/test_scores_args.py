"""The feature scores' call in the header, the ctypes table and the built library; every refusal it makes before anything is launched --
invalid-argument status with the call's name in mf_last_error() --; and every refusal of `ops.feature_scores` and of the stabilizer's
`cropping_and_distortion_resident`.  The C refusals and what Python decides before it reaches a device need no GPU; the rest is marked gpu."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = 'mf_feature_scores_f64'
P = 5


def test_library_exports_the_call():
    from meshflow_amd import _lib
    header = open(os.path.join(REPO, 'include', 'meshflow_hip.h')).read()
    assert NAME in _lib.SIGNATURES and len(_lib.SIGNATURES[NAME][1]) == 7
    assert hasattr(_lib.lib, NAME)
    assert re.search(r'\bint %s\(' % NAME, header)
    block = header[header.index('the scores from tracked features'):header.index('int %s(' % NAME)]
    for text in ('mfs.py:1196-1212', 'tests/scores_model.py', 'MINIMUM', 'not np.linalg.eigvals', '0x7FC00000', 'MF_HFIT_OK', 'or null',
                 '{pairs scored, the first pair that was not scored or -1}', '256 strided partial sums', 'No atomics', 'one 256-lane workgroup',
                 '1 <= pairs <= MF_SCORES_MAX_PAIRS', '1,048,576', 'Asynchronous on `stream`'):
        assert text in block, text
    assert re.search(r'#define MF_SCORES_MAX_PAIRS %d\b' % _lib.SCORES_MAX_PAIRS, header)
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import scores_model as sm
    assert sm.MAX_PAIRS == _lib.SCORES_MAX_PAIRS and sm.OK == _lib.HFIT_OK
    body = open(os.path.join(REPO, 'meshflow_amd', 'csrc', 'scores_body.h')).read()
    assert re.search(r'MAX_PAIRS = 1 << 20\b', body) and 1 << 20 == _lib.SCORES_MAX_PAIRS
    assert 'fma' not in body.replace('fused multiply-add', '') and 'fma' not in open(os.path.join(REPO, 'meshflow_amd', 'csrc', 'scores.hip')).read()
    makefile = open(os.path.join(REPO, 'meshflow_amd', 'csrc', 'Makefile')).read()
    assert re.search(r'^SRCS = .*\bscores\.hip\b', makefile, re.M) and re.search(r'^HDRS = .*\bscores_body\.h\b', makefile, re.M)
    assert '-ffp-contract=off' in makefile


@pytest.fixture(scope='module')
def env():
    from meshflow_amd import _lib
    buf = (ctypes.c_uint8 * (5 * 4096 + 64))()
    base = (ctypes.addressof(buf) + 15) & ~15
    return _lib, buf, base


def refused(_lib, *args):
    rc = getattr(_lib.lib, NAME)(*args)
    err = _lib.lib.mf_last_error()
    assert rc == _lib.MF_ERR_INVALID_ARG, (args, rc, err)
    assert NAME.encode() + b':' in err, err
    return err


def test_c_refusals(env):
    """Host addresses throughout, and no GPU needed: a call that got as far as a launch would not return MF_ERR_INVALID_ARG."""
    _lib, buf, base = env
    vp = ctypes.c_void_p
    # 4 KB apart: h is P * 72 = 360 bytes, info 80, pair 40, scores 8, record 8
    at = {k: base + 4096 * i for i, k in enumerate(('h', 'info', 'pair', 'scores', 'record'))}
    good = dict(n=P, **at)

    def call(**kw):
        a = dict(good, **kw)
        return (vp(a['h']), vp(a['info']), a['n'], vp(a['pair']), vp(a['scores']), vp(a['record']), None)

    for key in ('h', 'pair', 'scores', 'record'):
        assert b'null' in refused(_lib, *call(**{key: None})), key
        assert b'null' in refused(_lib, *call(**{key: None, 'info': None})), key
    for n in (0, -1, -(1 << 31)):
        assert b'no pair' in refused(_lib, *call(n=n)), n
    for n in (_lib.SCORES_MAX_PAIRS + 1, 1 << 30, (1 << 31) - 1):
        assert b'too many' in refused(_lib, *call(n=n)), n
    assert b'1 .. 1048576' in refused(_lib, *call(n=0))
    assert b'aligned' in refused(_lib, *call(h=at['h'] + 4))
    for key in ('info', 'pair', 'scores', 'record'):
        assert b'aligned' in refused(_lib, *call(**{key: at[key] + 2})), key
    for kw in (dict(pair=at['h'] + 8), dict(scores=at['h'] + P * 72 - 4), dict(record=at['info']), dict(pair=at['info'] + P * 16 - 4),
               dict(record=at['h'])):
        assert b'aliases' in refused(_lib, *call(**kw)), kw
    for kw in (dict(scores=at['pair'] + P * 8 - 4), dict(record=at['pair']), dict(record=at['scores'] + 4), dict(scores=at['record'] + 4)):
        assert b'alias' in refused(_lib, *call(**kw)), kw
    assert bytes(buf) == bytes(len(buf))                                # nothing was written anywhere


def test_python_refusals_before_the_library():
    torch = pytest.importorskip('torch')
    from meshflow_amd import ops
    from meshflow_amd.stabilizer import MeshFlowStabilizer
    h = torch.zeros((P, 3, 3), dtype=torch.float64)
    with pytest.raises(ValueError, match='homographies must be a CUDA/HIP'):
        ops.feature_scores(h)
    with pytest.raises(ValueError, match='homographies must be a CUDA/HIP'):
        ops.feature_scores(h.numpy(), None)
    s = MeshFlowStabilizer(mesh_row_count=4, mesh_col_count=4)
    clip = torch.zeros((3, 48, 64), dtype=torch.uint8)
    # unequal shapes: before any launch (these are host tensors; a launch would fail differently)
    for other in (torch.zeros((3, 24, 32), dtype=torch.uint8), torch.zeros((2, 48, 64), dtype=torch.uint8), torch.zeros((3, 64, 48), dtype=torch.uint8)):
        with pytest.raises(ValueError, match="need the crop at the clip's own size"):
            s.cropping_and_distortion_resident(clip, other)
    for bad in (clip.float(), clip[..., None].expand(3, 48, 64, 3), clip.numpy(), clip[0]):
        with pytest.raises(ValueError, match='must be a one-channel uint8 tensor'):
            s.cropping_and_distortion_resident(bad, clip)
        with pytest.raises(ValueError, match='must be a one-channel uint8 tensor'):
            s.cropping_and_distortion_resident(clip, bad)
    with pytest.raises(ValueError, match=r'the pair \(d_y, d_uv\)'):
        s.stabilize_scored((clip, clip, clip))


@pytest.mark.gpu
def test_python_refusals_on_the_device():
    torch = pytest.importorskip('torch')
    from meshflow_amd import ops
    if not torch.cuda.is_available():
        pytest.fail('no GPU visible: the -m gpu tests must run on an MI355X')
    dev = torch.device('cuda:0')
    h = torch.eye(3, dtype=torch.float64, device=dev).repeat(P, 1, 1)
    info = torch.zeros((P, 4), dtype=torch.int32, device=dev)

    def no(match, *args):
        with pytest.raises(ValueError, match=match):
            ops.feature_scores(*args)

    no('dtype', h.float())
    no('dtype', h, info.long())
    no('CUDA/HIP', h, info.cpu())
    no(r'must have shape \(P, 3, 3\)', h.reshape(P, 9))
    no(r'must have shape \(P, 3, 3\)', h[0])
    no(r'must have shape \(P, 3, 3\)', h.reshape(P, 3, 3, 1))
    no(r'info must have shape \(5, 4\)', h, info[:-1])
    no(r'info must have shape \(5, 4\)', h, info.reshape(-1))
    no('contiguous', torch.zeros((P, 3, 6), dtype=torch.float64, device=dev)[:, :, ::2])
    no('contiguous', h, torch.zeros((P, 8), dtype=torch.int32, device=dev)[:, ::2])
    no('no pair to score', h[:0])
    no('no pair to score', h[:0], info[:0])
    no('too many', torch.zeros(((1 << 20) + 1, 3, 3), dtype=torch.float64, device=dev))
    scores, per_pair, record = ops.feature_scores(h, info)
    assert scores.cpu().numpy().tolist() == [1.0, 1.0] and record.cpu().numpy().tolist() == [P, -1] and ops.feature_scores_check(record) is None
    assert np.array_equal(per_pair.cpu().numpy(), np.ones((P, 2), np.float32))
    assert np.array_equal(h.cpu().numpy(), np.stack([np.identity(3)] * P)) and not info.cpu().numpy().any()
