"""Per-kernel ISA comparison of two builds of libhanabi_hip.so (no GPU needed): every kernel symbol of OLD is disassembled from
both libraries' gfx950 code objects (llvm-objdump --offloading, then -d) and compared instruction by instruction; addresses,
encodings and alignment padding are ignored. Prints the symbols that differ or are missing, then a count; exit status 1 if any.
Usage: isa_diff.py OLD.so NEW.so     (e.g. the parent commit's build against this one)"""
import glob
import os
import re
import shutil
import subprocess
import sys
import tempfile

OBJDUMP = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "llvm-objdump")


def kernels(so):
    d = tempfile.mkdtemp()
    try:
        shutil.copy(so, os.path.join(d, "lib.so"))
        subprocess.run([OBJDUMP, "--offloading", "lib.so"], cwd=d, capture_output=True, check=True)
        out = {}
        for co in sorted(glob.glob(os.path.join(d, "lib.so.*gfx950"))):
            txt = subprocess.run([OBJDUMP, "-d", "--no-show-raw-insn", "--no-leading-addr", co], capture_output=True, text=True,
                                 check=True).stdout
            cur = None
            for line in txt.splitlines():
                m = re.match(r"^([0-9a-f]+ )?<(.+)>:$", line)
                if m:
                    cur = out.setdefault(m.group(2), [])
                    continue
                ins = re.sub(r"//.*$", "", line).strip()
                if cur is not None and ins and ins != "...":
                    cur.append(re.sub(r"<[^>]*\+0x[0-9a-f]+>", "<L>", ins))
        return out
    finally:
        shutil.rmtree(d, ignore_errors=True)


def main():
    old, new = kernels(sys.argv[1]), kernels(sys.argv[2])
    bad = 0
    for k in sorted(old):
        if new.get(k) != old[k]:
            print(("DIFF " if k in new else "MISSING ") + k)
            bad += 1
    print(f"{len(old)} symbols in the old build: {len(old) - bad} identical, {bad} differ or are missing; "
          f"{len(set(new) - set(old))} new symbols")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
