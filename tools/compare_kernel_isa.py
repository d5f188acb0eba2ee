"""Are the kernels of two checkouts the same machine code?  No GPU needed: hipcc cross-compiles gfx950 to assembly.

    python tools/compare_kernel_isa.py PARENT_CHECKOUT THIS_CHECKOUT [--units a.hip b.hip ...] [--json out.json]

Every unit of the list that exists in a checkout is compiled with the flags of reindexer_amd.build.HIP_FLAGS (without -shared, include paths
of that checkout) and `-S --cuda-device-only`.  A kernel's text runs from its label to the directive that opens its descriptor, i.e. through
its last instruction; it is compared by mangled name, whichever unit holds it, so code that moved between units compares against itself.
`.LBB<n>_<m>` / `.Lfunc_end<n>` labels (and the `BB<n>_<m>` of the loop comments) carry the function's ordinal inside its unit, which changes
when code moves: the ordinal is dropped first, and runs of blanks become one.  The text is only compared, never interpreted.  Prints one line per kernel: identical, changed, gone (parent only) or new."""
from __future__ import annotations

import argparse
import json
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
from reindexer_amd.build import HIP_FLAGS, HIPCC  # noqa: E402

DEFAULT_UNITS = ["knn_scan.hip", "knn_merge.hip", "knn_filter.hip", "knn_range.hip", "knn_scan_i6.hip", "knn_scan_i8.hip",
                 "ft_merge.hip", "ft_ranges.hip", "ft_admit.hip", "ft_finish.hip", "ft_transfer.hip", "ft_sparse.hip", "ft_phrase.hip"]
ORDINAL = re.compile(r"(\.L|\b)(BB|func_end|func_begin|tmp)\d+")   # (the loop comments name blocks as BB<n>_<m>, without the .L)


def assembly(checkout: Path, unit: Path, tmp: Path) -> str:
    flags = [f for f in HIP_FLAGS if f != "-shared" and not f.startswith("-I")]
    flags += [f"-I{checkout / 'include'}", f"-I{checkout / 'reindexer_amd' / 'csrc'}"]
    out = tmp / f"{checkout.name}_{unit.stem}.s"
    subprocess.run([HIPCC, *flags, "-S", "--cuda-device-only", str(unit), "-o", str(out)], check=True)
    return out.read_text()


def kernels(asm: str) -> dict[str, str]:
    """mangled kernel name -> its text with the per-unit ordinals dropped"""
    lines = asm.splitlines()
    names = {m.group(1) for line in lines if (m := re.match(r"\s*\.amdhsa_kernel\s+(\S+)", line))}
    out, cur, body = {}, None, []
    for line in lines:
        if cur is None:
            m = re.match(r"(\S+):", line)   # (the compiler puts a comment behind the label)
            if m and m.group(1) in names:
                cur, body = m.group(1), []
            continue
        if line.lstrip().startswith(".section"):   # the kernel's descriptor follows its last instruction
            out[cur] = "\n".join(body)
            cur = None
            continue
        # (runs of blanks to one: the comment column behind a label moves with the label's width)
        body.append(re.sub(r"\s+", " ", ORDINAL.sub(lambda m: m.group(1) + m.group(2), line)).strip())
    return out


def checkout_kernels(checkout: Path, units: list[str], tmp: Path) -> dict[str, tuple[str, str]]:
    """mangled kernel name -> (unit, text) over the units the checkout has"""
    have = [checkout / "reindexer_amd" / "csrc" / u for u in units]
    have = [u for u in have if u.exists()]
    jobs = min(len(have), int(os.environ.get("MAX_JOBS", 8))) or 1
    with ThreadPoolExecutor(max_workers=jobs) as ex:
        texts = list(ex.map(lambda u: assembly(checkout, u, tmp), have))
    found = {}
    for unit, text in zip(have, texts):
        for name, body in kernels(text).items():
            assert name not in found, f"{name} in {found[name][0]} and {unit.name}"
            found[name] = (unit.name, body)
    return found


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("parent", type=Path)
    ap.add_argument("this", type=Path)
    ap.add_argument("--units", nargs="+", default=DEFAULT_UNITS)
    ap.add_argument("--json", type=Path, help="write the verdicts there as well")
    args = ap.parse_args()
    with tempfile.TemporaryDirectory() as t:
        (Path(t) / "a").mkdir()
        (Path(t) / "b").mkdir()
        a = checkout_kernels(args.parent.resolve(), args.units, Path(t) / "a")
        b = checkout_kernels(args.this.resolve(), args.units, Path(t) / "b")
    verdicts = {}
    for name in sorted(set(a) | set(b)):
        if name not in b:
            verdict = "gone"
        elif name not in a:
            verdict = "new"
        else:
            verdict = "identical" if a[name][1] == b[name][1] else "changed"
        verdicts[name] = {"verdict": verdict, "parent_unit": a[name][0] if name in a else None, "unit": b[name][0] if name in b else None}
        print(f"{verdict:9s} {name}")
    counts = {v: sum(1 for k in verdicts.values() if k["verdict"] == v) for v in ("identical", "changed", "gone", "new")}
    print(counts)
    if args.json:
        args.json.write_text(json.dumps({"units": args.units, "counts": counts, "kernels": verdicts}, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
