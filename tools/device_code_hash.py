"""Hashes the device code of every translation unit, so that a host-side refactor can show that no kernel moved.

    python tools/device_code_hash.py SCRATCH_DIR

Compiles each file of build.SOURCES with build.FLAGS into SCRATCH_DIR, dumps the object's .hip_fatbin section (the
gfx950 code object bundle) with llvm-objcopy and prints `<source> <sha256> <bytes>`.  Needs no GPU.  Run it on two
trees and diff the tables: host-only edits leave every line as it is.
"""
import hashlib
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gi-gs_amd"))
import build  # noqa: E402

OBJCOPY = os.path.join(os.path.dirname(os.path.dirname(build.HIPCC)), "llvm", "bin", "llvm-objcopy")


def fatbin_hash(src: str, scratch: str):
    obj = os.path.join(scratch, src.replace(".hip", ".o"))
    fatbin = obj[:-2] + ".hip_fatbin"
    # hipcc derives a unit's id (the __hip_cuid_* symbol, also in the device code) from the source's absolute path: pin it,
    # or two checkouts of the same source differ
    subprocess.run([build.HIPCC, *build.FLAGS, "-cuid=" + src, "-c", os.path.join(build.CSRC, src), "-o", obj], check=True,
                   capture_output=True)
    subprocess.run([OBJCOPY, "--dump-section", ".hip_fatbin=" + fatbin, obj], check=True)
    data = open(fatbin, "rb").read()
    return src, hashlib.sha256(data).hexdigest(), len(data)


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    scratch = sys.argv[1]
    os.makedirs(scratch, exist_ok=True)
    with ThreadPoolExecutor(max_workers=6) as ex:
        for src, digest, size in ex.map(lambda s: fatbin_hash(s, scratch), build.SOURCES):
            print(src, digest, size)


if __name__ == "__main__":
    main()
