// ORACLE -- TEST INFRASTRUCTURE ONLY.  The LocalBA oracle (orb_ba_oracle.cpp) a second time, with the compiler
// free to contract a * b + c into fused multiply-adds: oracle_local_ba_contracted[_trace].  The arithmetic is the
// same; every contracted operation rounds once instead of twice.  It is a second valid rounding of the
// reference that, unlike reordering the edges, reaches the operations inside one edge and inside the solve --
// and it is the kind of rounding the device code has (orb_ba.hip contracts).  tests/ba_cases.py uses it to
// tell whether a problem is conditioned well enough to be held to the parity bars; nothing else calls it.
#pragma GCC optimize("fp-contract=fast")
#define oracle_g2o oracle_g2o_contracted
#define oracle_local_ba oracle_local_ba_contracted
#define oracle_local_ba_stop_after oracle_local_ba_contracted_stop_after
#define oracle_local_ba_trace oracle_local_ba_contracted_trace
#include "orb_ba_oracle.cpp"
