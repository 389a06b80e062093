"""Static instruction mix of the L-BFGS iteration-tail kernels, from one cross-compile of csrc/optimization.hip.

No GPU is needed: hipcc -S with the library's flags and -Rpass-analysis=kernel-resource-usage; the assembly of every
``lbfgs_iteration_tail*`` kernel is counted by instruction class.  Usage:
    python tools/tail_isa_stats.py [--out profiles/<name>.txt]
"""

from __future__ import annotations

import argparse
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from curobo_amd import build as B  # noqa: E402

ADDR64 = ("v_lshl_add_u64", "v_lshlrev_b64", "v_mad_u64_u32", "v_mad_i64_i32", "v_add_co_u32", "v_addc_co_u32", "v_ashrrev_i64")


def demangle(names):
    out = subprocess.run(["/opt/rocm/llvm/bin/llvm-cxxfilt"] if os.path.exists("/opt/rocm/llvm/bin/llvm-cxxfilt") else ["c++filt"],
                         input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
    return dict(zip(names, out))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    src = os.path.join(B.CSRC, "optimization.hip")
    with tempfile.TemporaryDirectory() as tmp:
        asm = os.path.join(tmp, "optimization.s")
        cmd = [B.hipcc_path(), *B._flags(), *B.NO_SLP, "--cuda-device-only", "-S", "-Rpass-analysis=kernel-resource-usage", "-x", "hip", src, "-o", asm]
        remarks = subprocess.run(cmd, capture_output=True, text=True, check=True).stderr
        text = open(asm).read()
    # resource remarks: "Function Name: X", "VGPRs: n", "ScratchSize [bytes/lane]: n", "Occupancy [waves/SIMD]: n"
    res, cur = {}, None
    for line in remarks.split("\n"):
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = res.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+(VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\d+)", line)
        if m and cur is not None:
            cur[m.group(1).split(" ")[0]] = int(m.group(2))
    rows = []
    for m in re.finditer(r"^(_Z\w*lbfgs_iteration_tail\w*):[^\n]*\n(.*?)^\.Lfunc_end", text, flags=re.S | re.M):
        name, body = m.group(1), m.group(2)
        ops = [ln.split()[0] for ln in body.split("\n") if ln.startswith("\t") and not ln.strip().startswith((".", ";"))]
        c = lambda pred: sum(1 for o in ops if pred(o))  # noqa: E731
        rows.append((name, res.get(name, {}), {
            "VALU": c(lambda o: o.startswith("v_")), "SALU": c(lambda o: o.startswith("s_") and not o.startswith(("s_waitcnt", "s_nop", "s_load", "s_cbranch", "s_branch", "s_endpgm"))),
            "loads": c(lambda o: o.startswith(("global_load", "flat_load"))), "stores": c(lambda o: o.startswith(("global_store", "flat_store"))),
            "addr64": c(lambda o: o.startswith(ADDR64)), "branches": c(lambda o: o.startswith("s_cbranch")),
            "saddr_loads": len(re.findall(r"^\tglobal_load_\w+ v\d+, v\d+, s\[", body, flags=re.M)),
            "total": len(ops)}))
    names = demangle([r[0] for r in rows])
    lines = ["kernel | VGPRs | scratch B/lane | waves/SIMD | VALU | SALU | loads (scalar-base) | stores | 64-bit VALU address ops | s_cbranch | instructions"]
    for name, r, k in sorted(rows, key=lambda r: names[r[0]]):
        short = re.sub(r"curobo_hip::|\(.*", "", names[name]).replace("void ", "")
        lines.append(f"{short} | {r.get('VGPRs', '?')} | {r.get('ScratchSize', '?')} | {r.get('Occupancy', '?')} | {k['VALU']} | {k['SALU']} | "
                     f"{k['loads']} ({k['saddr_loads']}) | {k['stores']} | {k['addr64']} | {k['branches']} | {k['total']}")
    out = "\n".join(lines) + "\n"
    sys.stdout.write(out)
    if args.out:
        with open(args.out, "w") as f:
            f.write(out)


if __name__ == "__main__":
    main()
