"""diagnostic only: where kmeans_kernel (one workgroup) spends its time on the large node of the 4K bench frame's first split round,
per phase (build with tools/build_dbg.sh: -DRHCCQ_KM_STAMPS in k7_kmeans.hip -> dbg_build/librhccq_kmdbg.so; thread 0 of problem 0
reads the 100 MHz wall clock at the phase boundaries).  python tools/kmstamps.py [reps]"""
import ctypes
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from roibasedimagecompression_amd import _lib
_lib.LIB_PATH = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "dbg_build", "librhccq_kmdbg.so")
from roibasedimagecompression_amd.ops import Rhccq
from kmeansbench import frame_node

rh = Rhccq(0)
keys, k = frame_node(rh)
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
out = (ctypes.c_ulonglong * 8)()
rh._raw.rhccq_debug_km_stamps.argtypes = [ctypes.c_void_p, ctypes.c_int]
rh.set_option(Rhccq.OPT_KMEANS_WIDE_PAIRS, 0)
rh.kmeans_split([keys], [k])
assert rh._raw.rhccq_debug_km_stamps(out, 1) == 0
for _ in range(reps):
    labs, info = rh.kmeans_split([keys], [k], return_info=True)
assert rh._raw.rhccq_debug_km_stamps(out, 1) == 0
us = np.array(list(out), dtype=np.float64) / 100.0 / reps
names = ["load, mean, tolerance", "k-means++", "E-step", "M-step without empty clusters", "empty-cluster branch", "final labelling"]
print(f"n {len(keys)} k {k}: {int(info[0][0])} Lloyd iterations, strict {int(info[0][1])}; thread 0 of the workgroup, us per call over {reps} calls")
for n, v in zip(names, us):
    print(f"  {n:32s} {v:9.1f} us  {100 * v / us[:6].sum():5.1f} %")
print(f"  {'sum':32s} {us[:6].sum():9.1f} us")
