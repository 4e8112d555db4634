"""Compare the device code of two builds of csrc/*.hip kernel by kernel, without a GPU:

    python tools/compare_device_code.py PARENT_DIR RESULT_DIR

Each directory holds NAME.s per source, written by ``hipcc <the Makefile's flags> -S --cuda-device-only -o DIR/NAME.s NAME.hip`` (as
tools/kernel_resources_json.py compiles).  Per kernel symbol (mangled names, so the argument structs' names count) the instruction text between the
symbol's label and its ``.Lfunc_end`` (local labels without the function's position in the file), the kernel descriptor and the metadata entry (registers, spills, scratch, static LDS, kernarg size, arguments) must be equal.  Prints
the number of kernels compared and every line outside the kernels' bodies and metadata that differs; exit status 1 if any kernel differs.

A change that merges or renames kernels gives its map from parent symbols to result symbols as repeated ``--rename OLD=NEW``, OLD and NEW substrings of
the mangled names (``--rename 14mlp_jvp_kernelILi0EEEvNS_10MlpJvpArgsE=18mlp_tangent_kernelILi0ENS_10MlpJvpArgsEEEvT0_``): every OLD in the parent's assembly
is read as NEW before the kernels are paired.  A symbol that no OLD names is paired exactly as before."""
import argparse
import collections
import glob
import os
import re
import sys


def split(text):
    """({symbol: instructions + kernel descriptor}, {symbol: metadata entry}, the remaining lines)"""
    # (local labels carry the position of their function in the file -- .LBB9_3, .Lfunc_end9 --, which moves with the order of instantiation,
    # and the compiler's comments repeat it: comments are dropped)
    text = re.sub(r'[ \t]*;.*$', '', re.sub(r'\.(LBB|Lfunc_begin|Lfunc_end)\d+', r'.\1', text), flags=re.M)
    found = re.search(r'^amdhsa\.kernels:\n(.*?)^amdhsa\.target', text, re.M | re.S)
    meta = {}
    if found:      # (a source without kernels has no such section)
        meta = {re.search(r'^\s+\.name:\s+(\S+)', entry, re.M).group(1): entry for entry in re.split(r'^  - ', found.group(1), flags=re.M)[1:]}
        text = text[:found.start(1)] + text[found.end(1):]
    bodies, rest, lines, i = {}, [], text.split('\n'), 0
    while i < len(lines):
        label, descriptor = re.match(r'^(\S+):$', lines[i]), re.match(r'^\s+\.amdhsa_kernel (\S+)', lines[i])
        if label and label.group(1) in meta or descriptor:
            end = '.Lfunc_end' if label else '\t.end_amdhsa_kernel'
            j = i + 1
            while not lines[j].startswith(end):
                j += 1
            symbol = label.group(1) if label else descriptor.group(1)
            bodies[symbol] = bodies.get(symbol, '') + '\n'.join(lines[i:j]) + '\n'
            i = j
            continue
        rest.append(lines[i])
        i += 1
    return bodies, meta, rest


def renamed(text, renames):
    """The parent's assembly with every OLD replaced by NEW: the symbol's label, descriptor, metadata entry and any reference to it alike."""
    for old, new in renames:
        text = text.replace(old, new)
    return text


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument('parent')
    parser.add_argument('result')
    parser.add_argument('--rename', action='append', default=[], metavar='OLD=NEW')
    args = parser.parse_args()
    parent, result, renames = args.parent, args.result, [tuple(pair.split('=', 1)) for pair in args.rename]
    compared, differ = 0, []
    for path in sorted(glob.glob(os.path.join(parent, '*.s'))):
        name = os.path.basename(path)
        (b0, m0, r0), (b1, m1, r1) = split(renamed(open(path).read(), renames)), split(open(os.path.join(result, name)).read())
        if sorted(b0) != sorted(b1) or sorted(m0) != sorted(m1):
            differ.append('%s: kernels %s' % (name, sorted(set(b0) ^ set(b1)) + sorted(set(m0) ^ set(m1))))
        for symbol in sorted(set(b0) & set(b1)):
            compared += 1
            if b0[symbol] != b1[symbol]:
                differ.append('%s: instructions or descriptor of %s' % (name, symbol))
            if m0.get(symbol) != m1.get(symbol):
                differ.append('%s: metadata of %s' % (name, symbol))
        # outside the kernels (directives, device functions that were not inlined, the compiler's identification): as multisets, since the order in
        # which templates are instantiated may move whole kernels
        c0, c1 = collections.Counter(r0), collections.Counter(r1)
        for line, sign in [(line, '-') for line in (c0 - c1).elements()] + [(line, '+') for line in (c1 - c0).elements()]:
            print('%s: non-code line differs: %s%s' % (name, sign, line))
        print('%s: %d kernels' % (name, len(set(b0) & set(b1))))
    print('%d kernels compared, %d differences' % (compared, len(differ)))
    for line in differ:
        print(line)
    return 1 if differ else 0


if __name__ == '__main__':
    sys.exit(main())
