"""Child process of the plan tests: reads [[N, n, m, ms, ns_max, cus, per_cu, tier_attr_ok, per_cu_tier], ...] as JSON on stdin and prints
daqp_amd_describe_plan's line for each under the environment it was started with.  Loads the library with ctypes alone: no device is touched."""
import ctypes as C
import json
import os
import sys

L = C.CDLL(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "daqp_amd", "lib", "libdaqp_amd.so"))
L.daqp_amd_describe_plan.argtypes = [C.c_int] * 9 + [C.c_char_p, C.c_int]
buf = C.create_string_buffer(8192)
out = []
for args in json.load(sys.stdin):
    L.daqp_amd_describe_plan(*args, buf, 8192)
    out.append(buf.value.decode())
sys.stdout.write("\n".join(out))
