"""k_gemm_k320's workgroup -> (row stream, 320-column group) mapping (csrc/sdn_gemm_k320.h, through the host entry
sdn_gemm_k320_map): every (stream, column group) is owned by exactly one workgroup -- a pair owned twice or never would not show
up as a launch error -- and the sibling workgroups of a stream, which read the same activation panels, share wg % 8: one XCD
under round-robin dealing.  No GPU needed."""
import ctypes as C

import pytest

import safe_denoiser_amd as sda


def mapping(grid, ncg):
    lib = sda.lib()
    out, S = [], None
    for wg in range(grid):
        s, c = C.c_int32(-7), C.c_int32(-7)
        n = lib.sdn_gemm_k320_map(grid, ncg, wg, C.byref(s), C.byref(c))
        assert S is None or n == S, "the stream count must not depend on the workgroup asked about"
        S = n
        out.append((s.value, c.value))
    return S, out


@pytest.mark.parametrize("ncg", [1, 2, 3])
@pytest.mark.parametrize("grid", [255, 256, 304, 17, 24, 3, 2, 1])
def test_every_pair_once_and_siblings_share_an_xcd(grid, ncg):
    S, m = mapping(grid, ncg)
    per_xcd = [len(range(x, grid, 8)) // ncg for x in range(8)]
    assert S == sum(per_xcd)                                             # every XCD seats as many whole sibling sets as it can
    owners = {}
    for wg, (s, c) in enumerate(m):
        if s < 0:
            continue
        assert 0 <= s < S and 0 <= c < ncg
        assert (s, c) not in owners, f"({s}, {c}) owned by workgroups {owners[(s, c)]} and {wg}"
        owners[(s, c)] = wg
    assert len(owners) == S * ncg                                        # ... and every pair is owned
    for s in range(S):
        assert len({owners[(s, c)] % 8 for c in range(ncg)}) == 1, f"stream {s}: siblings on different XCDs"
    idle = sum(1 for s, _ in m if s < 0)
    assert idle == grid - S * ncg and idle < 8 * ncg                     # fewer than one sibling set per XCD is left over


def test_full_chip_counts():
    assert mapping(256, 1)[0] == 256 and mapping(256, 3)[0] == 80        # N = 960 on 256 CUs: 240 workgroups work, 16 have none
    assert mapping(17, 3)[0] == 1 and mapping(16, 3)[0] == 0             # one stream of three siblings needs workgroups 0, 8, 16


def test_bad_arguments():
    lib = sda.lib()
    s, c = C.c_int32(), C.c_int32()
    assert lib.sdn_gemm_k320_map(0, 1, 0, C.byref(s), C.byref(c)) < 0
    assert lib.sdn_gemm_k320_map(8, 0, 0, C.byref(s), C.byref(c)) < 0
    assert lib.sdn_gemm_k320_map(8, 1, 8, C.byref(s), C.byref(c)) < 0
    assert lib.sdn_gemm_k320_map(8, 1, 7, None, None) == 8
