"""the sub-step loop of a kernel in a hipcc -S file: the innermost backward-branch loop that holds N v_div_fmas (default 7), counted by
kind.  python tools/loop_stats.py file.s kernel-name-substring [n_div_fmas] [--print]   (whole-kernel figures: tools/isa_stats.py)"""
import re
import sys

lines = open(sys.argv[1]).read().split('\n')
pat = sys.argv[2]
want = int(sys.argv[3]) if len(sys.argv) > 3 and sys.argv[3].isdigit() else 7
INSTR = re.compile(r'(v_|s_|ds_|global_|buffer_|scratch_|flat_)')

start = None
for i, l in enumerate(lines):
    m = re.match(r'^(_Z\w+):', l)
    if m and start is not None:
        end = i
        break
    if m and pat in m.group(1):
        start, name = i, m.group(1)
else:
    end = len(lines)
if start is None:
    sys.exit(f"no kernel matches {pat}")
body = lines[start:end]
labels = {m.group(1): i for i, l in enumerate(body) for m in [re.match(r'^(\.LBB\w+):', l)] if m}
best = None
for i, l in enumerate(body):
    m = re.match(r'\s+s_cbranch_\w+\s+(\.LBB\w+)', l) or re.match(r'\s+s_branch\s+(\.LBB\w+)', l)
    if m and labels.get(m.group(1), i) < i:
        lo = labels[m.group(1)]
        ins = [t.strip() for t in body[lo:i + 1] if INSTR.match(t.strip())]
        if sum(t.startswith('v_div_fmas') for t in ins) == want and (best is None or len(ins) < len(best[2])):
            best = (lo, i, ins)
if best is None:
    sys.exit(f"no backward-branch loop with {want} v_div_fmas in {name}")
lo, hi, ins = best
op = lambda p: sum(t.startswith(p) for t in ins)
print(name[:100])
print(f"  loop: lines {start + lo + 1}..{start + hi + 1}  instr {len(ins)}  valu {op('v_')}  packed {op('v_pk_')}  v_mov {op('v_mov')}  "
      f"s_nop {op('s_nop')}  s_waitcnt {op('s_waitcnt')}  salu {sum(t.startswith('s_') and not t.startswith(('s_nop', 's_waitcnt')) for t in ins)}")
print(f"  v_div_scale {op('v_div_scale')}  v_rcp {op('v_rcp')}  v_div_fmas {op('v_div_fmas')}  v_div_fixup {op('v_div_fixup')}  "
      f"v_sqrt/rsq {op('v_sqrt') + op('v_rsq')}")
if '--print' in sys.argv:
    print('\n'.join(body[lo:hi + 1]))
