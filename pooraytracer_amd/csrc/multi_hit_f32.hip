// multi_hit_f32.hip — K7 (multi_hit.hip) in the fp32 fast mode (PRT_PRECISION_F32): every real number a float, the 48-byte
// records and the node array fp32 K1 walks.  Rays, cursors and hits stay fp64 records at the boundary; a cursor's t is
// rounded to float on load, and since a hit's t is a widened float, paging is exact in fp32 as well.  Launcher in namespace
// prt32.
#define PRT_REAL float
#define PRT_F32_TU 1
#include "multi_hit.hip"
