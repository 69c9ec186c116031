"""No GPU: the six side-plane calls in the header, the ctypes table and the built library, and every refusal they make before anything is
launched -- invalid-argument status with the call's name in mf_last_error()."""
import ctypes
import os
import re

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = {'mf_warp_plane_f32': 12, 'mf_warp_plane_nearest': 13, 'mf_crop_resize_plane_f32': 13, 'mf_crop_resize_plane_nearest': 14,
         'mf_crop_resize_dev_plane_f32': 11, 'mf_crop_resize_dev_plane_nearest': 12}


def test_library_exports_the_plane_calls():
    from meshflow_amd import _lib
    header = open(os.path.join(REPO, 'include', 'meshflow_hip.h')).read()
    for name, nargs in CALLS.items():
        assert name in _lib.SIGNATURES, name
        assert len(_lib.SIGNATURES[name][1]) == nargs, name
        assert hasattr(_lib.lib, name), name
        assert re.search(r'\bint %s\(' % name, header), name
    assert 'mfs.py:1063-1069' in header[header.index('side planes'):header.index('int mf_warp_plane_f32(')]
    assert _lib.lib.mf_abi_version() == 1


@pytest.fixture(scope='module')
def env():
    from meshflow_amd import _lib
    buf = (ctypes.c_uint8 * 256)()
    base = (ctypes.addressof(buf) + 15) & ~15
    return _lib, buf, base


def refused(_lib, name, *args):
    rc = getattr(_lib.lib, name)(*args)
    err = _lib.lib.mf_last_error()
    assert rc == _lib.MF_ERR_INVALID_ARG, (name, args, rc)
    assert name.encode() in err, (name, err)
    return err


def test_warp_plane_refusals(env):
    _lib, buf, base = env
    p, q = ctypes.c_void_p(base), ctypes.c_void_p(base + 64)
    good = dict(n=3, W=64, H=48, R=4, C=4)

    def f32(planes=p, out=q, table=p, crop=p, bounds=None, **kw):
        a = dict(good, **kw)
        return ('mf_warp_plane_f32', planes, out, table, a['n'], a['W'], a['H'], a['R'], a['C'], 1.5, crop, bounds, None)

    def nn(planes=p, out=q, table=p, crop=p, bounds=None, es=4, **kw):
        a = dict(good, **kw)
        return ('mf_warp_plane_nearest', planes, out, table, a['n'], a['W'], a['H'], a['R'], a['C'], es, 7, crop, bounds, None)

    for call in (f32, nn):
        for kw in (dict(planes=None), dict(out=None), dict(table=None), dict(crop=None)):
            assert b'null' in refused(_lib, *call(**kw))
        assert b'alias' in refused(_lib, *call(out=p))
        for kw in (dict(n=0), dict(n=-2), dict(W=1), dict(H=1), dict(W=32768), dict(H=32768), dict(W=0), dict(R=65), dict(C=65), dict(R=0), dict(C=-1)):
            refused(_lib, *call(**kw))
    for es in (0, 3, 5, 16, -1):
        assert b'elem_bytes' in refused(_lib, *nn(es=es))
    # a plane or output pointer that is not aligned to its element
    assert b'aligned' in refused(_lib, *f32(planes=ctypes.c_void_p(base + 2)))
    assert b'aligned' in refused(_lib, *f32(out=ctypes.c_void_p(base + 65)))
    for es, off in ((2, 1), (4, 2), (8, 4)):
        assert b'aligned' in refused(_lib, *nn(es=es, planes=ctypes.c_void_p(base + off)))
        assert b'aligned' in refused(_lib, *nn(es=es, out=ctypes.c_void_p(base + 64 + off)))


def test_crop_resize_plane_refusals(env):
    _lib, buf, base = env
    p, q = ctypes.c_void_p(base), ctypes.c_void_p(base + 64)
    good = dict(n=3, W=64, H=48, oW=64, oH=48, rect=(2, 3, 60, 40))

    def host(nearest, planes=p, out=q, work=p, es=4, **kw):
        a = dict(good, **kw)
        head = (planes, out, a['n'], a['W'], a['H']) + tuple(a['rect']) + (a['oW'], a['oH'])
        return ('mf_crop_resize_plane_nearest',) + head + (es, work, None) if nearest else ('mf_crop_resize_plane_f32',) + head + (work, None)

    def dev(nearest, planes=p, out=q, work=p, bounds=p, status=p, es=4, **kw):
        a = dict(good, **kw)
        head = (planes, out, a['n'], a['W'], a['H'], bounds, a['oW'], a['oH'])
        return (('mf_crop_resize_dev_plane_nearest',) + head + (es, work, status, None) if nearest
                else ('mf_crop_resize_dev_plane_f32',) + head + (work, status, None))

    for nearest in (False, True):
        for call in (host, dev):
            for kw in (dict(planes=None), dict(out=None), dict(work=None)):
                assert b'null' in refused(_lib, *call(nearest, **kw))
            assert b'alias' in refused(_lib, *call(nearest, out=p))
            for kw in (dict(n=0), dict(W=0), dict(H=0), dict(W=32768), dict(H=32768)):
                assert b'shape' in refused(_lib, *call(nearest, **kw))
            for kw in (dict(oW=0), dict(oH=0), dict(oW=32768), dict(oH=-3)):
                assert b'output size' in refused(_lib, *call(nearest, **kw))
            assert b'aligned' in refused(_lib, *call(nearest, planes=ctypes.c_void_p(base + 2)))
            assert b'aligned' in refused(_lib, *call(nearest, out=ctypes.c_void_p(base + 66)))
        for kw in (dict(bounds=None), dict(status=None)):
            assert b'null' in refused(_lib, *dev(nearest, **kw))
        for rect in ((5, 3, 4, 40), (2, 9, 60, 8), (-1, 3, 60, 40), (2, 3, 64, 40), (2, 3, 60, 48)):
            assert b'rectangle' in refused(_lib, *host(nearest, rect=rect))
    for call in (host, dev):
        for es in (0, 3, 6, 16):
            assert b'elem_bytes' in refused(_lib, *call(True, es=es))
        assert b'aligned' in refused(_lib, *call(True, es=8, planes=ctypes.c_void_p(base + 4)))
    assert bytes(buf) == bytes(256)                    # nothing was written anywhere


def test_python_refusals_before_the_library():
    """What `ops.warp_planes` / `ops.crop_resize_planes` decide on their own needs no device: CPU tensors are refused first of all."""
    torch = pytest.importorskip('torch')
    import types
    from meshflow_amd import ops
    table = types.SimpleNamespace(n=2, W=8, H=4, R=1, C=1)
    with pytest.raises(ValueError):
        ops.warp_planes(torch.zeros((2, 4, 8)), table)
    with pytest.raises(ValueError):
        ops.warp_planes(torch.zeros((2, 4, 8)), table, interpolation='cubic')
    with pytest.raises(ValueError):
        ops.crop_resize_planes(torch.zeros((2, 4, 8)), (0, 0, 7, 3))
