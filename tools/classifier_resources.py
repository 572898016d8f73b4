"""Register / scratch / occupancy table of the classifier kernels (compiler remarks; no GPU needed): the fp32 instantiations of
classifier.hip, the bf16 ones of classifier_bf16.hip and the row-selected ones of classifier_rows.hip ("rows"), one line per kernel,
element type of X / dX last.
usage: python tools/classifier_resources.py [unit.hip ...] [extra hipcc flags]
  (default units: h2gcn_amd/csrc/classifier.hip, classifier_bf16.hip, classifier_rows.hip; name another file -- e.g. an older
   commit's classifier.hip -- to put its table next to this one)"""
import re
import subprocess
import sys
import tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
units = [a for a in sys.argv[1:] if a.endswith(".hip")]
flags = [a for a in sys.argv[1:] if not a.endswith(".hip")]
if not units:
    units = [str(ROOT / "h2gcn_amd/csrc" / u) for u in ("classifier.hip", "classifier_bf16.hip", "classifier_rows.hip")]
KERNEL = re.compile(r"(small_fwd_kernel|small_dx_kernel|dropout_dense_fwd_kernel|dropout_dense_dx_kernel|dropout_dense_dw_kernel|"
                    r"pack_w_fwd_kernel|pack_w_dx_kernel|reduce_dw_kernel)((?:ILi\d+E(?:Li\d+E)?)?)(f|NS_4bf16E)?(?:Lb([01])E)?")
for unit in units:
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-fPIC", f"-I{ROOT}/include", f"-I{ROOT}/h2gcn_amd/csrc", "--offload-arch=gfx950",
               "--cuda-device-only", "-c", "-Rpass-analysis=kernel-resource-usage", unit, "-o", f"{tmp}/k.o"] + flags
        txt = subprocess.run(cmd, capture_output=True, text=True).stderr
    print(f"# {Path(unit).name}")
    rows = []
    for b in re.split(r"remark: [^\n]*Function Name: ", txt)[1:]:
        name = b.split("\n")[0].strip()

        def g(k):
            m = re.search(k + r": (\d+)", b)
            return int(m.group(1)) if m else -1
        m = KERNEL.search(name)
        if not m:
            continue
        ints = re.findall(r"Li(\d+)E", m.group(2))
        label = m.group(1) + ("<" + ", ".join(ints) + ">" if ints else "") + {None: "", "f": " f32", "NS_4bf16E": " bf16"}[m.group(3)] + (" rows" if m.group(4) == "1" else "")
        scratch, occ, lds = g(r"ScratchSize \[bytes/lane\]"), g(r"Occupancy \[waves/SIMD\]"), g(r"LDS Size \[bytes/block\]")
        rows.append(f"{label:40s} vgpr {g('VGPRs'):3d} agpr {g('AGPRs'):3d} sgpr {g('SGPRs'):3d} scratch {scratch:3d} occupancy {occ} lds {lds}")
    print("\n".join(sorted(rows)))
