"""sha256 digests of the gfx950 device code in built objects or libraries.

    python scripts/device_code_digest.py build/net_c4.hip.o [more .o / .so ...]

Prints one JSON document: per input file and per gfx950 code object in it, the
sha256 of the .text, .rodata (kernel descriptors) and .note (kernel metadata)
sections, and per kernel symbol the sha256 of its bytes.  Two builds with equal
digests run the same device code.  (The whole code object is not compared: its
string tables hold a compilation-unit id that hashes the source text.)

It only hashes bytes: nothing is disassembled."""
import hashlib
import json
import os
import subprocess
import sys
import tempfile

from kernel_regs import B, code_objects

SECTIONS = (".text", ".rodata", ".note")


def digest(co):
    """{sections: {name: {size, sha256}}, kernels: {symbol: {size, sha256}}} of one code object"""
    elf = open(co, "rb").read()
    sha = lambda b: hashlib.sha256(b).hexdigest()
    doc = json.loads(subprocess.run([f"{B}/llvm-readelf", "--elf-output-style=JSON", "-S", "-s", co],
                                    capture_output=True, text=True, check=True).stdout)[0]
    secs = {s["Section"]["Name"]["Name"]: s["Section"] for s in doc["Sections"]}
    text = secs[".text"]
    res = {"sections": {}, "kernels": {}}
    for n in SECTIONS:
        s = secs[n]
        res["sections"][n] = {"size": s["Size"], "sha256": sha(elf[s["Offset"]:s["Offset"] + s["Size"]])}
    for ent in doc["Symbols"]:
        sym = ent["Symbol"]
        if sym["Type"]["Name"] != "Function" or sym["Section"]["Name"] != ".text":
            continue
        off = text["Offset"] + sym["Value"] - text["Address"]
        res["kernels"][sym["Name"]["Name"]] = {"size": sym["Size"], "sha256": sha(elf[off:off + sym["Size"]])}
    res["kernels"] = dict(sorted(res["kernels"].items()))
    return res


def main():
    out = {}
    for path in sys.argv[1:]:
        with tempfile.TemporaryDirectory() as t:
            out[os.path.basename(path)] = [digest(co) for co in code_objects(path, t)]
    json.dump(out, sys.stdout, indent=1, sort_keys=True)
    print()


if __name__ == "__main__":
    main()
