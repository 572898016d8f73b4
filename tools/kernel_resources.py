"""Register / scratch / occupancy table of every kernel in h2gcn_capi.hip, spmm_short.hip and spmm_bf16.hip (compiler remarks;
no GPU needed).  spmm_hops_kernel rows end in the gather-source / output element types (f32 / bf16).
usage: python tools/kernel_resources.py [--used-in profile.txt ...] [extra hipcc flags]
       python tools/kernel_resources.py --compare <checkout of the parent commit> [extra hipcc flags]
  --compare: EVERY kernel of EVERY translation unit of the library, the parent checkout against this tree (see compare())
  --used-in: print only the spmm_hops_kernel instantiations whose (demangled) names appear in the given rocprofv3-derived
             profile texts (profiles/*_epoch_*.txt, *_train_step_*.txt, *_kernel_stats.csv ...), with the ms / calls columns of
             the line they appear in -- i.e. the resources of the kernels a workload REALLY dispatched."""
import re
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent


def compare(parent: Path, flags) -> None:
    """--compare <tree>: every kernel of every translation unit of libh2gcn_hip.so (SRCS of csrc/Makefile), the checkout at
    <tree> (the parent commit) against this tree: which kernels keep every reported figure, which differ, which are new."""
    from concurrent.futures import ThreadPoolExecutor

    fields = ("TotalSGPRs", "VGPRs", "AGPRs", r"ScratchSize \[bytes/lane\]", r"Occupancy \[waves/SIMD\]", r"LDS Size \[bytes/block\]",
              "SGPRs Spill", "VGPRs Spill")

    def remarks(job):
        tree, unit = job
        cmd = ["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-fPIC", f"-I{tree}/include", "--offload-arch=gfx950", "--cuda-device-only",
               "-c", "-Rpass-analysis=kernel-resource-usage", str(tree / "h2gcn_amd/csrc" / unit), "-o", "/dev/null"] + list(flags)
        out = {}
        for b in re.split(r"remark: [^\n]*Function Name: ", subprocess.run(cmd, capture_output=True, text=True).stderr)[1:]:
            out[(unit, b.split("\n")[0].split()[0])] = tuple(int(re.search(r"\b" + k + r": (\d+)", b).group(1)) for k in fields)
        return out

    def units(tree):
        return re.search(r"^SRCS\s*:=\s*(.*)$", (tree / "h2gcn_amd/csrc/Makefile").read_text(), flags=re.M).group(1).split()

    jobs = [(parent, u) for u in units(parent)] + [(ROOT, u) for u in units(ROOT)]
    with ThreadPoolExecutor(8) as pool:
        res = list(pool.map(remarks, jobs))
    old, new = {}, {}
    for (tree, _), r in zip(jobs, res):
        (old if tree == parent else new).update(r)
    same = [k for k in old if new.get(k) == old[k]]
    diff = [k for k in old if k in new and new[k] != old[k]]
    gone = [k for k in old if k not in new]
    fresh = [k for k in new if k not in old]
    print(f"kernels in the parent build: {len(old)}   in this build: {len(new)}")
    print(f"identical in every reported figure: {len(same)}   different: {len(diff)}   missing: {len(gone)}   new: {len(fresh)}")
    head = "(SGPRs VGPRs AGPRs scratch occupancy LDS sgpr_spill vgpr_spill)"

    def line(v, k):
        return " ".join(f"{x:6d}" for x in v) + f"  {k[1]}"
    print(f"\nNEW KERNELS {head}")
    for k in fresh:
        print(line(new[k], k))
    if diff or gone:
        print(f"\nDIFFERENT OR MISSING: parent line, then this tree's {head}")
        for k in diff + gone:
            print(line(old[k], k))
            if k in new:
                print(line(new[k], k))
    print(f"\nEXISTING KERNELS, parent == this tree {head}")
    for k in same:
        print(line(old[k], k))


if "--compare" in sys.argv:
    at = sys.argv.index("--compare")
    compare(Path(sys.argv[at + 1]).resolve(), sys.argv[1:at] + sys.argv[at + 2:])
    sys.exit(0)
DTYPE = {None: "f32", "float": "f32", "f": "f32", "h2gcn::bf16": "bf16", "NS_4bf16E": "bf16", "S1_": "bf16"}  # (S1_: the mangled back-reference to bf16)
used = {}
argv = sys.argv[1:]
while "--used-in" in argv:
    i = argv.index("--used-in")
    j = i + 1
    while j < len(argv) and not argv[j].startswith("-"):
        for line in Path(argv[j]).read_text().splitlines():
            m = re.search(r"spmm_hops_kernel<(\d+), (\d+), (true|false), (true|false), (true|false), (true|false), (true|false), (true|false), (\d+)"
                          r"(?:, (true|false))?(?:, (float|h2gcn::bf16), (float|h2gcn::bf16))?(?:, (?:true|false))?>", line)
            if m:
                key = tuple("1" if v == "true" else "0" if v in ("false", None) else DTYPE.get(v, v) for v in m.groups())
                used.setdefault(key, []).append(f"{Path(argv[j]).name}: {' '.join(line.split()[-2:])}")
        j += 1
    del argv[i:j]
sys.argv[1:] = argv
txt = ""
for unit in ("h2gcn_capi.hip", "spmm_short.hip", "spmm_bf16.hip"):      # the translation units that hold spmm_hops_kernel instantiations
    if not (ROOT / "h2gcn_amd/csrc" / unit).exists():
        continue
    cmd = ["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-fPIC", f"-I{ROOT}/include", "--offload-arch=gfx950",
           "--cuda-device-only", "-c", "-Rpass-analysis=kernel-resource-usage", str(ROOT / "h2gcn_amd/csrc" / unit),
           "-o", "/tmp/_kres.o"] + sys.argv[1:]
    txt += subprocess.run(cmd, capture_output=True, text=True).stderr
for b in re.split(r"remark: [^\n]*Function Name: ", txt)[1:]:
    name = b.split("\n")[0].strip()

    def g(k):
        m = re.search(k + r": (\d+)", b)
        return int(m.group(1)) if m else -1
    m = re.search(r"spmm_hops_kernelILi(\d+)ELi(\d+)ELb(\d)ELb(\d)ELb(\d)ELb(\d)ELb(\d)ELb(\d)ELi(\d+)ELb(\d)E(f|NS_4bf16E)?(f|S1_)?(?:Lb(\d)E)?", name)
    rowval = bool(m) and m.group(13) == "1"      # the row-constant mode (last template parameter)
    if m:
        m_groups = m.groups()[:10] + tuple(DTYPE[t] for t in m.groups()[10:12])
    if used and not (m and m_groups in used):
        continue
    where = ("   <- " + "; ".join(used[m_groups])) if used and m else ""
    if m:
        v, lpr, ex, su, o32, pipe, sh, epi, fb, lists, ts, td = m_groups
        name = f"spmm<VEC{v} LPR{lpr:>2s} {'EXACT' if ex=='1' else 'tiled'} {'SUM' if su=='1' else 'fwd'} {'off32' if o32=='1' else 'off64'}" \
               f"{' PIPE' if pipe=='1' else ''}{' SHORT' if sh=='1' else ''}{' LISTS' if lists=='1' else ''}{' GEN' if epi=='1' else ''} FB{fb}" \
               f"{'' if ts == td == 'f32' else f' {ts}->{td}'}{' ROWVAL' if rowval else ''}>"
    scratch, occ = g(r"ScratchSize \[bytes/lane\]"), g(r"Occupancy \[waves/SIMD\]")
    print(f"{name:64s} vgpr {g('VGPRs'):3d} sgpr {g('SGPRs'):3d} scratch {scratch:3d} occupancy {occ}{where}")
