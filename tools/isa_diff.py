""" Which kernels of two builds of libgpp_hip.so (or of two object files) differ in their gfx950 code (no GPU needed):

    python tools/isa_diff.py path/to/old.so path/to/new.so

Every kernel symbol of the OLD build is looked up in the NEW one and its disassembly compared instruction by instruction (addresses
and the encodings are dropped: a kernel that only moved inside its code object is the same kernel).  Prints the symbols that changed
or disappeared, and how many are new; exit code 1 when a symbol of the old build changed or is gone.  A change that adds a form of a
kernel as a compile-time switch (the ragged stem, gpp_conv2d_preact) shows with it that the kernels that existed kept their code.
"""
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import isa_audit  # noqa: E402


def kernels_of(path):
    """ {symbol: [instruction text, ...]} over all gfx950 code objects of the file """
    out = {}
    for _, image in isa_audit.code_objects(path):
        with tempfile.NamedTemporaryFile(suffix='.co', delete=False) as f:
            f.write(image)
            tmp = f.name
        try:
            dis = subprocess.run([os.path.join(isa_audit.LLVM, 'llvm-objdump'), '-d', '--no-show-raw-insn', '--no-leading-addr', tmp],
                                 stdout=subprocess.PIPE, universal_newlines=True, check=True).stdout
        finally:
            os.unlink(tmp)
        func = None
        for line in dis.splitlines():
            m = re.match(r'^(?:[0-9a-f]+ )?<(.+)>:$', line)
            if m:
                func = m.group(1)
                out[func] = []
                continue
            text = re.sub(r'//.*$', '', line).strip()
            if func and text:
                out[func].append(text)
    return out


def main(argv):
    if len(argv) != 2:
        print(__doc__)
        return 2
    old, new = kernels_of(argv[0]), kernels_of(argv[1])
    if not old or not new:
        print('isa_diff: no gfx950 kernel found in one of the files: nothing was compared')
        return 1
    gone = sorted(k for k in old if k not in new)
    changed = sorted(k for k in old if k in new and old[k] != new[k])
    pretty = isa_audit.demangle(gone + changed)
    print('{} symbols in the old build: {} unchanged, {} changed, {} gone; {} new'.format(
        len(old), len(old) - len(gone) - len(changed), len(changed), len(gone), sum(1 for k in new if k not in old)))
    for k in changed:
        print('  CHANGED ({} -> {} instructions)  {}'.format(len(old[k]), len(new[k]), pretty[k][:160]))
    for k in gone:
        print('  GONE  {}'.format(pretty[k][:160]))
    return 1 if (gone or changed) else 0


if __name__ == '__main__':
    sys.exit(main(sys.argv[1:]))
