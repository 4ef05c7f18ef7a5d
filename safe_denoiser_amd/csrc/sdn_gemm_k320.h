// Workgroup -> (row stream, column group) of k_gemm_k320 (sdn_gemm_k320.hip), shared by the kernel and the host
// (sdn_gemm_k320_map, tests/test_k320_map.py).
#pragma once

#if defined(__HIPCC__)
#define SDN_K320_HD __host__ __device__
#else
#define SDN_K320_HD
#endif

// Workgroups are dealt round-robin over the 8 XCDs (workgroup b runs on XCD b % 8 of the dealing; which physical XCD that is does
// not matter here), and the ncg sibling workgroups of a row stream -- one per 320-column group, all reading the same activation
// panels -- should share an XCD's L2.  So XCD x's workgroups x, x + 8, x + 16, ... are cut into runs of ncg: run j of XCD x is one
// stream, its members the column groups 0 .. ncg - 1; streams are numbered XCD by XCD.  Workgroups left over at the end of an
// XCD's list (fewer than ncg) get stream -1 and exit.  Returns the number of streams S; every (stream < S, column group) is
// owned by exactly one workgroup.
SDN_K320_HD inline int sdn_k320_map(int grid, int ncg, int wg, int* stream, int* cgroup) {
  const int x = wg & 7, y = wg >> 3;
  int S = 0, base = 0;
  for (int xx = 0; xx < 8; ++xx) {
    const int cnt = (grid - xx + 7) >> 3;                    // workgroups of the grid on XCD xx
    if (xx == x) base = S;
    S += cnt / ncg;
  }
  const int per = ((grid - x + 7) >> 3) / ncg;               // streams on this workgroup's XCD
  const int sl = y / ncg;
  *cgroup = y - sl * ncg;
  *stream = sl < per ? base + sl : -1;
  return S;
}
