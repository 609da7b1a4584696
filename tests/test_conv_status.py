"""Status codes of the Glow conv entry points (csrc/conv1x1.hip, csrc/conv3x3_1x1.hip) for unsupported shapes, bad
sizes, NULL and misaligned pointers, one fault and two faults at a time (two faults pin the order of the checks), and
the full tables of their *_supported / *_pack_floats functions.  No GPU needed: every call either fails validation or
has an empty batch, so nothing is launched; the pointers are never dereferenced.  A case with a non-empty batch always
carries a fault that validation must catch, and the test refuses to call one that is expected to pass.

EXPECTED and TABLE_SHA256 were recorded, called in this way, from the library built at the commit before the two
units' dispatch and validation moved onto csrc/host_common.hpp (launch_listed, aligned, all_aligned).  The literals
are that build's answers, and the test passes on that build as it does on the present one: the move kept every status."""
import ctypes
import hashlib

import pytest

import vcnf_amd

FAKE = 0x1000            # 16-byte aligned, never dereferenced
OFF4 = 0x1004            # 4 bytes off a 16-byte boundary
W2_FLOATS = 8 * 16 * 2 * 64 * 4


def _p(v):
    return ctypes.c_void_p(v) if v else None


def _conv1x1(L, a):
    floats = L.vcnf_conv1x1_pack_floats(32, 40) + a.get("wf", 0)
    return L.vcnf_conv1x1_f16x3_f32(_p(a.get("x", FAKE)), _p(a.get("y", FAKE)), _p(a.get("w", FAKE)), floats, None, None,
                                    a.get("batch", 0), a.get("c_in", 32), a.get("c_out", 40), a.get("inner", 4), 1, 0.01,
                                    1, 0.01, None, None)


def _conv3x3_1x1(L, a):
    w1f = L.vcnf_conv3x3_1x1_pack_floats(3) + a.get("w1f", 0)
    return L.vcnf_conv3x3_1x1_f16x3_f32(_p(a.get("x", FAKE)), _p(a.get("y", FAKE)), _p(a.get("w1", FAKE)), w1f,
                                        _p(a.get("w2", FAKE)), W2_FLOATS + a.get("w2f", 0), None, None, a.get("batch", 0),
                                        a.get("c_in", 3), a.get("h", 2), a.get("w", 2), 0.01, 0.01, None, None)


def _taps(L, a):
    w1f = L.vcnf_conv3x3_1x1_pack_floats(3) + a.get("w1f", 0)
    w3f = L.vcnf_convnet3_w3_pack_floats(6) + a.get("w3f", 0)
    return L.vcnf_convnet3_taps_f16x3_f32(_p(a.get("x", FAKE)), _p(a.get("z", FAKE)), _p(a.get("w1", FAKE)), w1f,
                                          _p(a.get("w2", FAKE)), W2_FLOATS + a.get("w2f", 0), _p(a.get("w3", FAKE)), w3f,
                                          None, None, a.get("batch", 0), a.get("c_in", 3), a.get("c_out", 6), a.get("h", 2),
                                          a.get("w", 2), 0.01, 0.01, None, None)


def _col2im(L, a):
    return L.vcnf_col2im3x3_f32(_p(a.get("z", FAKE)), None, _p(a.get("out", FAKE)), a.get("batch", 0), a.get("c", 6),
                                a.get("h", 2), a.get("w", 2), None)


# entry point -> (call(L, changes), cases); a case is the changes to a valid call with an empty batch
ENTRY = {
    "vcnf_conv1x1_f16x3_f32": (_conv1x1, (
        dict(c_in=0), dict(c_in=17), dict(c_in=272), dict(c_out=0), dict(c_out=257),
        dict(batch=-1), dict(inner=0), dict(wf=1), dict(wf=-1),
        dict(),
        dict(batch=1, x=0), dict(batch=1, y=0), dict(batch=1, w=0),
        dict(batch=1, w=OFF4),
        dict(c_in=17, batch=-1), dict(c_out=257, wf=1), dict(batch=-1, x=0), dict(wf=1, batch=1, x=0),
        dict(c_in=17, batch=1, x=0), dict(batch=1, x=0, w=OFF4), dict(x=0, y=0, w=0), dict(w=OFF4),
    )),
    "vcnf_conv3x3_1x1_f16x3_f32": (_conv3x3_1x1, (
        dict(c_in=0), dict(c_in=25),
        dict(batch=-1), dict(h=0), dict(w=0), dict(w1f=1), dict(w1f=-1), dict(w2f=1), dict(w2f=-1),
        dict(),
        dict(batch=1, x=0), dict(batch=1, y=0), dict(batch=1, w1=0), dict(batch=1, w2=0),
        dict(batch=1, w1=OFF4), dict(batch=1, w2=OFF4),
        dict(c_in=25, batch=-1), dict(c_in=0, w1f=1), dict(h=0, x=0), dict(w2f=1, batch=1, x=0),
        dict(c_in=25, batch=1, y=0), dict(batch=1, y=0, w2=OFF4), dict(x=0, y=0, w1=0, w2=0), dict(w1=OFF4),
    )),
    "vcnf_convnet3_taps_f16x3_f32": (_taps, (
        dict(c_in=0), dict(c_in=25), dict(c_out=0), dict(c_out=57),
        dict(batch=-1), dict(h=0), dict(w=0), dict(w1f=1), dict(w1f=-1), dict(w2f=1), dict(w2f=-1), dict(w3f=1), dict(w3f=-1),
        dict(),
        dict(batch=1, x=0), dict(batch=1, z=0), dict(batch=1, w1=0), dict(batch=1, w2=0), dict(batch=1, w3=0),
        dict(batch=1, w1=OFF4), dict(batch=1, w2=OFF4), dict(batch=1, w3=OFF4),
        dict(c_out=57, batch=-1), dict(c_in=25, w3f=1), dict(w=0, z=0), dict(w3f=1, batch=1, x=0),
        dict(c_out=57, batch=1, z=0), dict(batch=1, z=0, w3=OFF4), dict(x=0, z=0, w1=0, w2=0, w3=0), dict(w3=OFF4),
    )),
    "vcnf_col2im3x3_f32": (_col2im, (
        dict(batch=-1), dict(c=0), dict(h=0), dict(w=0),
        dict(),
        dict(batch=1, z=0), dict(batch=1, out=0),
        dict(batch=-1, z=0), dict(c=0, batch=1, out=0), dict(z=0, out=0),
    )),
}

# one status per case, in the order of the cases; 0: the case reaches the return for an empty batch
EXPECTED = {
    "vcnf_conv1x1_f16x3_f32": (5, 5, 5, 5, 5, 2, 2, 2, 2, 0, 1, 1, 1, 3, 5, 5, 2, 2, 5, 1, 0, 0),
    "vcnf_conv3x3_1x1_f16x3_f32": (5, 5, 2, 2, 2, 2, 2, 2, 2, 0, 1, 1, 1, 1, 3, 3, 5, 5, 2, 2, 5, 1, 0, 0),
    "vcnf_convnet3_taps_f16x3_f32": (5, 5, 5, 5, 2, 2, 2, 2, 2, 2, 2, 2, 2, 0, 1, 1, 1, 1, 1, 3, 3, 3, 5, 5, 2, 2, 5, 1, 0, 0),
    "vcnf_col2im3x3_f32": (2, 2, 2, 2, 0, 1, 1, 2, 2, 0),
}


@pytest.mark.parametrize("entry", sorted(ENTRY))
def test_status_codes(entry):
    L = vcnf_amd.lib()
    call, cases = ENTRY[entry]
    assert len(EXPECTED[entry]) == len(cases)
    for case, want in zip(cases, EXPECTED[entry]):
        assert not (case.get("batch", 0) != 0 and want == 0), "only an empty batch may pass: nothing is launched here"
        assert call(L, case) == want, (entry, case)


def _tables(L):
    r = range(301)
    return {
        "conv1x1_supported": [L.vcnf_conv1x1_supported(i, o) for i in r for o in r],
        "conv1x1_pack_floats": [L.vcnf_conv1x1_pack_floats(i, o) for i in r for o in r],
        "conv3x3_1x1_supported": [L.vcnf_conv3x3_1x1_supported(i, h, o) for h in (255, 256, 257) for i in r for o in r],
        "conv3x3_1x1_pack_floats": [L.vcnf_conv3x3_1x1_pack_floats(i) for i in r],
        "convnet3_supported": [L.vcnf_convnet3_supported(i, h, o) for h in (255, 256, 257) for i in r for o in r],
        "convnet3_w3_pack_floats": [L.vcnf_convnet3_w3_pack_floats(o) for o in r],
    }


TABLE_SHA256 = {
    "conv1x1_supported": "ba188e57373fa40c18ece08ea104cde3e65cc10a27ce82e2f58be320b6d27275",
    "conv1x1_pack_floats": "4935986d8e75381d4b9f6e69b8227692c92f03dea8d0e189f8de1f21a773cdb4",
    "conv3x3_1x1_supported": "6e402cb3d3d803c66084c7edc2507d4ac203b99cbe21f11dcaf62fc876c00f0d",
    "conv3x3_1x1_pack_floats": "b8c74dee9a5a9c2ef5986af57c2ee71d4320194b55bca21192136f66514cb17b",
    "convnet3_supported": "a79eeabbcfa8d82603a8d3db742a7b9bb08fb4bb07f77f89d6500fa88d71ca2f",
    "convnet3_w3_pack_floats": "c46e7c01c59ca4d23f6abbbc0ec0e17228d42e2b373d59dccca378e725672c4f",
}


def test_supported_and_pack_tables():
    L = vcnf_amd.lib()
    t = _tables(L)
    r = range(301)
    # the definitions (include/vcnf_hip.h) ...
    ok1 = lambda i, o: 16 <= i <= 256 and i % 16 == 0 and 1 <= o <= 256
    assert t["conv1x1_supported"] == [int(ok1(i, o)) for i in r for o in r]
    assert t["conv1x1_pack_floats"] == [8 * (i // 16) * 2 * 64 * 4 if ok1(i, o) else 0 for i in r for o in r]
    assert t["conv3x3_1x1_supported"] == [int(1 <= i <= 24 and h == 256 and o == 256)
                                          for h in (255, 256, 257) for i in r for o in r]
    assert t["conv3x3_1x1_pack_floats"] == [8 * ((9 * i + 15) // 16) * 2 * 64 * 4 if 1 <= i <= 24 else 0 for i in r]
    assert t["convnet3_supported"] == [int(1 <= i <= 24 and h == 256 and 1 <= o <= 56)
                                       for h in (255, 256, 257) for i in r for o in r]
    assert t["convnet3_w3_pack_floats"] == [((9 * o + 31) // 32) * 16 * 2 * 64 * 4 if 1 <= o <= 56 else 0 for o in r]
    # ... and the recorded answers
    assert sorted(t) == sorted(TABLE_SHA256)
    for name, values in t.items():
        assert hashlib.sha256(",".join(map(str, values)).encode()).hexdigest() == TABLE_SHA256[name], name
