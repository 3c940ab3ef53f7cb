"""The SIMD roles of step pipelines (aad_amd.engine.SimdRoleAllocator, used by EncodeDecodePipeline), on the CPU: the four engines of
two live pipelines hold four different SIMDs, the two encoders on different halves of the LDS path ({0, 1} and {2, 3}); a
pipeline beyond that gets no role; closing a pipeline frees its slot for the next one.  A pipeline that is alive alone runs
without roles: they come into force with the second pipeline and go when either of the two closes."""
from aad_amd.engine import EncodeDecodePipeline, SimdRoleAllocator


class FakeEngine:
    def __init__(self):
        self.role = "unset"

    def set_simd_role(self, simd=None):
        self.role = simd


def fake_pipeline(alloc):
    """EncodeDecodePipeline's own use of the allocator, with the device work left out"""
    p = EncodeDecodePipeline.__new__(EncodeDecodePipeline)
    p.enc_engine, p.dec_engine = FakeEngine(), FakeEngine()
    p._take_simd_roles(alloc)
    return p


def roles(p):
    return (p.enc_engine.role, p.dec_engine.role)


def test_two_pipelines_hold_four_simds():
    a = SimdRoleAllocator()
    s0 = a.acquire()
    assert a.roles(s0) == (None, None) and not a.in_force()  # alone: no roles
    s1 = a.acquire()
    e0, d0 = a.roles(s0)
    e1, d1 = a.roles(s1)
    assert sorted((e0, d0, e1, d1)) == [0, 1, 2, 3]
    assert {e0 // 2, e1 // 2} == {0, 1}  # the encoders: one in {0, 1}, one in {2, 3}
    s2 = a.acquire()  # a fifth and sixth engine
    assert s2 is None and a.roles(s2) == (None, None)
    a.release(s2)  # releasing nothing is fine
    a.release(s0)
    assert a.roles(s1) == (None, None)
    assert a.acquire() == s0 and a.acquire() is None
    assert a.roles(s1) == (2, 3)
    a.release(s1)
    a.release(s0)
    a.release(s0)  # twice is once
    assert a.taken == [False, False] and a.holders == [None, None]


def test_pipelines_set_and_clear_their_engines_roles():
    alloc = SimdRoleAllocator()
    first = fake_pipeline(alloc)
    assert roles(first) == (None, None) and first._role_slot == 0  # alone: the engines are told "off"
    second = fake_pipeline(alloc)
    assert roles(first) == (0, 1) and roles(second) == (2, 3)  # four live engines, four SIMDs
    third = fake_pipeline(alloc)  # a fifth and sixth engine: off, the four keep theirs
    assert roles(third) == ("unset", "unset") and third._role_slot is None
    assert roles(first) == (0, 1) and roles(second) == (2, 3)
    third._release_simd_roles()  # it held nothing
    assert roles(first) == (0, 1) and roles(second) == (2, 3) and roles(third) == ("unset", "unset")
    first._release_simd_roles()
    first._release_simd_roles()  # twice is once
    assert roles(first) == (None, None) and roles(second) == (None, None) and alloc.taken == [False, True]
    fourth = fake_pipeline(alloc)  # the freed slot
    assert roles(fourth) == (0, 1) and roles(second) == (2, 3)
    second._release_simd_roles()
    fourth._release_simd_roles()
    assert roles(fourth) == (None, None) and alloc.taken == [False, False]
    off = fake_pipeline(None)  # roles switched off for this pipeline
    assert roles(off) == ("unset", "unset")
    off._release_simd_roles()
