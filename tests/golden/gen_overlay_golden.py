#!/usr/bin/env python3
"""The two colour lists the reference's detect_image paints its segmentation overlays with (achelous.py:134-142: `colors_seg` and, reversed, `colors_seg_line`),
read out of the reference's SOURCE: achelous.py imports cv2, which is not installed where the fixtures are made, so the module is parsed, not imported, and the
two literal lists are evaluated with ast.literal_eval.  Writes tests/golden/overlay_palettes.json.

    python tests/golden/gen_overlay_golden.py <directory of the reference checkout>"""
import ast
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))


def literal_lists(path):
    tree = ast.parse(open(path, encoding='utf-8').read())
    found = {}
    for node in ast.walk(tree):
        if isinstance(node, ast.Assign) and len(node.targets) == 1 and isinstance(node.targets[0], ast.Attribute) and node.targets[0].attr in ('colors_seg', 'colors_seg_line'):
            v, rev = node.value, False
            # colors_seg_line = list(reversed([...]))
            while isinstance(v, ast.Call) and isinstance(v.func, ast.Name) and v.func.id in ('list', 'reversed') and len(v.args) == 1:
                rev = rev or v.func.id == 'reversed'
                v = v.args[0]
            if isinstance(v, ast.List) and node.targets[0].attr not in found:
                lst = [list(c) for c in ast.literal_eval(v)]
                found[node.targets[0].attr] = lst[::-1] if rev else lst
    return found


if __name__ == '__main__':
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get('ACHELOUS_REFERENCE', '')
    lists = literal_lists(os.path.join(ref, 'achelous.py'))
    assert set(lists) == {'colors_seg', 'colors_seg_line'}, sorted(lists)
    assert lists['colors_seg_line'] == lists['colors_seg'][::-1]
    out = {'source': 'achelous.py:134-142', 'colors_seg': lists['colors_seg'], 'colors_seg_line': lists['colors_seg_line']}
    with open(os.path.join(HERE, 'overlay_palettes.json'), 'w') as fh:
        json.dump(out, fh)
        fh.write('\n')
    print('wrote overlay_palettes.json:', len(lists['colors_seg']), 'colours')
