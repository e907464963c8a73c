#!/usr/bin/env python3
"""Hash of the machine code of every device function of built objects, symbol by symbol: two builds whose listings are
equal run the same device code (the -S text is no such witness: its label numbers move with the instantiation order).
    python tools/kernel_hash.py build/hip/chain.o [build/hip/head.o ...]     -> "<object> <symbol> <bytes> <sha256/16>", sorted"""
import hashlib
import os
import re
import shutil
import subprocess
import sys
import tempfile

LLVM = '/opt/rocm/lib/llvm/bin'


def device_functions(obj):
    """{symbol: bytes of its instructions} of the gfx950 code object bundled into `obj`"""
    with tempfile.TemporaryDirectory() as tmp:
        local = os.path.join(tmp, os.path.basename(obj))
        shutil.copy(obj, local)
        subprocess.run([LLVM + '/llvm-objdump', '--offloading', local], check=True, stdout=subprocess.DEVNULL, cwd=tmp)
        elf = [f for f in os.listdir(tmp) if 'amdgcn' in f]
        if not elf:                          # a source without device code
            return {}
        run = lambda *cmd: subprocess.run(cmd + (os.path.join(tmp, elf[0]),), check=True, capture_output=True, text=True).stdout
        text, symtab = run(LLVM + '/llvm-objdump', '-d'), run(LLVM + '/llvm-readelf', '-sW')
    # a symbol's own size: what the disassembly shows behind it up to the next symbol is alignment padding
    size = {f[7]: int(f[2]) for f in map(str.split, symtab.splitlines()) if len(f) == 8 and f[3] == 'FUNC'}
    out, name = {}, None
    for line in text.splitlines():
        m = re.match(r'^[0-9a-f]+ <(.+)>:$', line)
        if m:
            name = m.group(1)
            out[name] = bytearray()
            continue
        m = re.search(r'// [0-9A-F]+: ((?:[0-9A-F]{8} ?)+)', line)      # the instruction's dwords after its address
        if m and name is not None:
            out[name] += bytes.fromhex(m.group(1).replace(' ', ''))
    return {n: bytes(c[:size[n]]) for n, c in out.items()}


for obj in sys.argv[1:]:
    for name, code in sorted(device_functions(obj).items()):
        print(os.path.basename(obj), name, len(code), hashlib.sha256(code).hexdigest()[:16])
