"""Compare the gfx950 code objects of two builds of one HIP object, kernel by kernel.

    python tools/code_object_diff.py A.o B.o

Both objects are unbundled (tools/kernel_resources.py) and disassembled.  Reported: the functions present
in only one of the two, the functions whose instruction text differs -- addresses and encodings dropped,
branch targets renamed to labels numbered within their function -- and the count of identical ones.
Exit status 1 on any difference: a change to host code alone leaves every kernel as it was.
"""
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from kernel_resources import LLVM, code_object  # noqa: E402


def functions(obj):
    """{symbol: [instruction text, ...]} of the object's gfx950 code."""
    with tempfile.TemporaryDirectory() as td:
        co = code_object(obj, td)
        isa = subprocess.run([f"{LLVM}/llvm-objdump", "-d", "--symbolize-operands", "--no-show-raw-insn", co],
                             capture_output=True, text=True, check=True).stdout
    out = {}
    body = None
    labels = {}
    for line in isa.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:\s*$", line)
        if m and not re.fullmatch(r"L\d+", m.group(1)):
            body = out.setdefault(m.group(1), [])
            labels = {}
            continue
        if body is None or not line.strip() or line.strip() == "...":   # (...: zero padding between functions)
            continue
        if m:   # a branch target: the disassembler numbers them through the whole object
            body.append(labels.setdefault(m.group(1), f"T{len(labels)}") + ":")
            continue
        text = re.sub(r"\s*//.*$", "", line).strip()
        text = re.sub(r"\bL\d+\b", lambda t: labels.setdefault(t.group(0), f"T{len(labels)}"), text)
        body.append(text)
    return out


def main():
    if len(sys.argv) != 3:
        raise SystemExit(__doc__)
    a, b = functions(sys.argv[1]), functions(sys.argv[2])
    only_a = sorted(set(a) - set(b))
    only_b = sorted(set(b) - set(a))
    differ = sorted(k for k in set(a) & set(b) if a[k] != b[k])
    for k in only_a:
        print(f"only in {sys.argv[1]}: {k}")
    for k in only_b:
        print(f"only in {sys.argv[2]}: {k}")
    for k in differ:
        n = next((i for i, (x, y) in enumerate(zip(a[k], b[k])) if x != y), min(len(a[k]), len(b[k])))
        print(f"differs: {k} ({len(a[k])} / {len(b[k])} lines, first at line {n})")
    same = len(set(a) & set(b)) - len(differ)
    print(f"{same} identical, {len(differ)} differing, {len(only_a)} + {len(only_b)} in one object only")
    return 1 if only_a or only_b or differ else 0


if __name__ == "__main__":
    sys.exit(main())
