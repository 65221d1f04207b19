"""Per-kernel register / scratch / occupancy summary of libkalibr_hip (hipcc -Rpass-analysis=kernel-resource-usage).

usage: python tools/resource_usage.py [filter-substring] [extra hipcc flags...]
A filter that contains "k_sp" reads kb_spline.hip instead of kb_capi.hip; one that contains "k_build" reads the nine
build units (kb_build_tu.hip -DKB_TU_ID=0..8), e.g. `python tools/resource_usage.py "k_buildp<"`.
"""
import re
import subprocess
import sys

sys.path.insert(0, __import__("os").path.join(__import__("os").path.dirname(__file__), ".."))
from kalibr_amd import build as B  # noqa: E402

flt = sys.argv[1] if len(sys.argv) > 1 else ""
extra = sys.argv[2:]
src = B.SRC_SPLINE if "k_sp" in flt else B.SRC  # the spline path's kernels are a translation unit of their own
if "k_build" in flt:  # the build kernels: the nine per-model-set units of kb_build_tu.hip, compiled side by side
    ps = [subprocess.Popen([B.HIPCC] + B.FLAGS + extra + ["-DKB_TU_ID=%d" % i, "-Rpass-analysis=kernel-resource-usage",
                                                          "-c", "-o", "/tmp/ru%d.o" % i, B.SRC_BUILD_TU],
                           stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True) for i in range(B.N_BUILD_TU)]
    stderr = "".join(p.communicate()[1] for p in ps)
else:
    stderr = subprocess.run([B.HIPCC] + B.FLAGS + extra + ["-Rpass-analysis=kernel-resource-usage", "-c", "-o",
                                                           "/tmp/ru.o", src], capture_output=True, text=True).stderr
cur = None
rows = {}
for line in stderr.splitlines():
    m = re.search(r"remark:\s+(.*?): (.*?) \[-Rpass", line)
    if not m:
        continue
    k, v = m.group(1).strip(), m.group(2).strip()
    if k == "Function Name":
        cur = v
        rows[cur] = {}
    elif cur:
        rows[cur][k] = v
keys = ["VGPRs", "AGPRs", "VGPRs Spill", "SGPRs Spill", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]"]
for fn, kv in rows.items():
    dem = subprocess.run(["c++filt", fn], capture_output=True, text=True).stdout.strip()
    if flt in dem:
        dem = dem.replace("void ", "").replace("(anonymous namespace)::", "")  # the build units' kernels
        print(f"{dem[:60]:60s} " + " ".join(f"{k.split(' [')[0].replace(' ', '_')}={kv.get(k, '-')}" for k in keys))
