// prt_probe_f32.hip — the fp32 twin of prt_probe.hip: every real a float, as in prt_kernels_f32.hip; launchers
// prtprobe_<op>_f32, plus the exhaustive fp32 checks that exist only here.
#define PRT_REAL float
#define PRT_PROBE_F32 1
#include "prt_probe.hip"
