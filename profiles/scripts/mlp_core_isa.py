"""Kernel set and resources of the register-chained MLP kernels (mlp_kernel, ffn2_kernel, pf_mlp_kernel, rv_mlp_kernel) in two builds of the engines' gfx950
assembly (`make isa` plus the same rule for engine_f32): the list of kernel symbols must be identical, and per instantiation the scratch size must not grow, the
LDS size and the allocated VGPRs (next_free_vgpr rounded up to the allocation granule of 8) must be equal.  Reads the .amdhsa_* metadata lines of each kernel
descriptor, counts the instruction lines of each kernel body and compares a hash of each body's text (comments dropped, basic-block label numbers made
anonymous) between the builds; it looks at no instruction's name.
usage: python profiles/scripts/mlp_core_isa.py BEFORE_BUILD_DIR AFTER_BUILD_DIR [--out profiles/mlp_core_isa.txt]      (exit status 1 when a rule is broken)"""
import argparse
import hashlib
import os
import re
import subprocess
import sys

ENGINES = ('engine_f32', 'engine_bf16', 'engine_f16')
FAMILIES = ('mlp_kernel', 'ffn2_kernel', 'pf_mlp_kernel', 'rv_mlp_kernel')
FIELDS = {'.amdhsa_private_segment_fixed_size': 'scratch', '.amdhsa_group_segment_fixed_size': 'lds', '.amdhsa_next_free_vgpr': 'vgpr',
          '.amdhsa_accum_offset': 'accum', '.amdhsa_next_free_sgpr': 'sgpr'}
LABEL = re.compile(r'^(_Z\w+):')
BLOCK = re.compile(r'\.LBB\d+_')


def scan(path):
    """{kernel symbol: {'instrs': n, 'scratch': .., 'lds': .., 'vgpr': .., 'accum': .., 'sgpr': ..}}"""
    out, body, desc = {}, None, None
    for line in open(path):
        m = LABEL.match(line)
        if m:
            body = m.group(1)
            out.setdefault(body, {'instrs': 0, 'text': hashlib.sha256()})
        elif line.startswith('.Lfunc_end'):
            out[body]['text'] = out[body]['text'].hexdigest()
            body = None
        elif line.startswith('\t.amdhsa_kernel '):
            desc = line.split()[1]
        elif line.startswith('\t.end_amdhsa_kernel'):
            desc = None
        elif desc is not None:
            f = line.split()
            if len(f) == 2 and f[0] in FIELDS:
                out[desc][FIELDS[f[0]]] = int(f[1])
        elif body is not None:
            out[body]['text'].update(BLOCK.sub('.LBB_', line.split(';')[0]).encode())
            if line.startswith('\t') and line[1:2].isalpha():
                out[body]['instrs'] += 1
    return {k: v for k, v in out.items() if 'vgpr' in v}          # kernels only (device functions have no descriptor)


def demangle(names):
    r = subprocess.run(['c++filt'], input='\n'.join(names), capture_output=True, text=True, check=True)
    return dict(zip(names, r.stdout.splitlines()))


def granule(v):
    return (v + 7) // 8 * 8


ap = argparse.ArgumentParser()
ap.add_argument('before')
ap.add_argument('after')
ap.add_argument('--out', default=None)
a = ap.parse_args()
lines, broken = [], []
for eng in ENGINES:
    old, new = scan(os.path.join(a.before, eng + '.s')), scan(os.path.join(a.after, eng + '.s'))
    same = sorted(old) == sorted(new)
    lines.append(f'{eng}: {len(old)} kernels before, {len(new)} after; symbol lists {"identical" if same else "DIFFER"}')
    if not same:
        broken.append(f'{eng}: kernel symbols differ: {sorted(set(old) ^ set(new))[:8]}')
    names = demangle(sorted(set(old) & set(new)))
    watched = [k for k in sorted(names, key=lambda k: names[k]) if any(names[k].startswith(f'void ach::{fam}<') for fam in FAMILIES)]
    outside = [names[k] for k in names if k not in watched and (old[k]['instrs'], old[k]['vgpr'], old[k]['lds'], old[k]['scratch']) != (new[k]['instrs'], new[k]['vgpr'], new[k]['lds'], new[k]['scratch'])]
    moved = [names[k] for k in names if old[k]['text'] != new[k]['text']]
    lines.append(f'  kernel bodies whose text differs: {len(moved)} of {len(names)}' + ''.join(f'\n    {n.split("(")[0]}' for n in moved))
    lines.append(f'  other kernels whose instruction count or resources changed: {len(outside)}' + ''.join(f'\n    {n}' for n in outside[:20]))
    lines.append(f'  {"kernel":58s} {"instrs":>13s} {"scratch":>9s} {"LDS":>13s} {"VGPR (granule)":>21s} {"accum":>9s} {"SGPR":>9s}')
    for k in watched:
        o, n = old[k], new[k]
        short = names[k][len('void ach::'):].split('(')[0].replace('ach::', '')
        lines.append(f'  {short:58s} {o["instrs"]:6d} {n["instrs"]:6d} {o["scratch"]:4d} {n["scratch"]:4d} {o["lds"]:6d} {n["lds"]:6d} '
                     f'{o["vgpr"]:4d} {n["vgpr"]:4d} ({granule(o["vgpr"]):3d} {granule(n["vgpr"]):3d}) {o["accum"]:4d} {n["accum"]:4d} {o["sgpr"]:4d} {n["sgpr"]:4d}')
        if n['scratch'] > o['scratch']:
            broken.append(f'{eng} {short}: scratch {o["scratch"]} -> {n["scratch"]}')
        if n['lds'] != o['lds']:
            broken.append(f'{eng} {short}: LDS {o["lds"]} -> {n["lds"]}')
        if granule(n['vgpr']) != granule(o['vgpr']):
            broken.append(f'{eng} {short}: allocated VGPRs {granule(o["vgpr"])} -> {granule(n["vgpr"])}')
lines.append('rules broken: ' + ('none' if not broken else ''.join('\n  ' + b for b in broken)))
text = '\n'.join(['columns: before after (instruction count, scratch bytes, LDS bytes, next_free_vgpr and its granule of 8, accum_offset, next_free_sgpr)'] + lines) + '\n'
sys.stdout.write(text)
if a.out:
    with open(a.out, 'w') as f:
        f.write(text)
sys.exit(1 if broken else 0)
