"""issue slots on the path ONE wave executes through a kernel of a hipcc -S file, per class, for the prologue (entry .. head of the
sub-step loop), the sub-step loop (one trip) and the epilogue (loop exit .. s_endpgm).

  python tools/path_stats.py file.s kernel-name-substring DECISIONS [--trips 8] [--n-div-fmas 7] [--explain]

DECISIONS: one letter per CONDITIONAL branch in the order the walk meets them outside the loop, T = taken, N = falls through
(e.g. NNTNT...).  The walk starts behind the compatibility header of a kernel with preloaded kernel arguments.  Unconditional branches are followed.  The sub-step loop is the innermost backward-branch loop that holds
--n-div-fmas v_div_fmas (tools/loop_stats.py's rule); its body is counted once, its back edge needs no letter, conditional branches
inside it are taken as falling through.  --explain prints every branch met with the instructions in front of it: that is how a regime's
letters are read off the .s (a letter the string does not have counts as N and is shown as `?`).
Classification is by mnemonic prefix only: v_mov | v_pk_ | other v_ | s_load | s_waitcnt | s_nop | branch (s_cbranch, s_branch) |
other s_ (SALU, s_endpgm included) | vmem (global_ buffer_ flat_ scratch_) | ds_.  "no compute" = v_mov + SALU + s_load + s_nop +
s_waitcnt + branch: slots that do no arithmetic, compare / select or memory access of the agent's data."""
import re
import sys

args = [a for a in sys.argv[1:] if not a.startswith('--')]
if len(args) < 2:
    sys.exit(__doc__)


def opt(name, default):
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


lines = open(args[0]).read().split('\n')
pat = args[1]
decisions = args[2] if len(args) > 2 else ''
trips, want, explain = opt('--trips', 8), opt('--n-div-fmas', 7), '--explain' in sys.argv
INSTR = re.compile(r'(v_|s_|ds_|global_|buffer_|scratch_|flat_)')
CLASSES = ['v_mov', 'v_pk', 'valu', 's_load', 's_waitcnt', 's_nop', 'branch', 'salu', 'vmem', 'ds']
IDLE = ('v_mov', 'salu', 's_load', 's_nop', 's_waitcnt', 'branch')


def klass(t):
    for p, k in (('v_mov', 'v_mov'), ('v_pk_', 'v_pk'), ('v_', 'valu'), ('s_load', 's_load'), ('s_waitcnt', 's_waitcnt'), ('s_nop', 's_nop'),
                 ('s_cbranch', 'branch'), ('s_branch', 'branch'), ('s_', 'salu'), ('ds_', 'ds')):
        if t.startswith(p):
            return k
    return 'vmem'


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
CB = re.compile(r'\s+s_cbranch_\w+\s+(\.LBB\w+)')
UB = re.compile(r'\s+s_branch\s+(\.LBB\w+)')
loop = None
for i, l in enumerate(body):
    m = CB.match(l) or UB.match(l)
    if m and labels.get(m.group(1), i) < i:
        lo = labels[m.group(1)]
        n = sum(t.strip().startswith('v_div_fmas') for t in body[lo:i + 1])
        if n == want and (loop is None or i - lo < loop[1] - loop[0]):
            loop = (lo, i)
if loop is None:
    sys.exit(f"no backward-branch loop with {want} v_div_fmas in {name}")

# a kernel built with preloaded kernel arguments opens with a compatibility header (s_load of the preloaded words, s_branch .LBBn_0, pad to
# 256 bytes) that the dispatcher skips where it preloads: the walk starts behind it
entry = 0
head = [(i, l.strip()) for i, l in enumerate(body) if INSTR.match(l.strip())][:8]
for i, t in head:
    m = UB.match(body[i])
    if m and all(x.startswith(('s_load', 's_waitcnt')) for j, x in head if j < i) and '.p2align\t8' in ''.join(body[i:labels[m.group(1)]]):
        entry = labels[m.group(1)]

counts = {ph: dict.fromkeys(CLASSES, 0) for ph in ('prologue', 'loop', 'epilogue')}
pc, k, phase, steps, used = entry, 0, 'prologue', 0, ''
while True:
    steps += 1
    if steps > 200000:
        sys.exit("the walk does not end: a backward branch outside the sub-step loop is taken")
    if pc >= len(body):
        sys.exit("fell off the end of the kernel")
    if pc == loop[0] and phase == 'prologue':
        phase = 'loop'
    t = body[pc].strip()
    if not INSTR.match(t):
        pc += 1
        continue
    counts[phase][klass(t)] += 1
    if t.startswith('s_endpgm'):
        break
    mc, mu = CB.match(body[pc]), UB.match(body[pc])
    if phase == 'loop':
        if pc == loop[1]:
            phase = 'epilogue'
            if mu:
                sys.exit("the loop ends in an unconditional branch: not a form this tool walks")
        pc += 1
        continue
    if mu:
        pc = labels[mu.group(1)]
        continue
    if mc:
        d = decisions[k] if k < len(decisions) else '?'
        k += 1
        used += d
        if explain:
            ctx = [x.strip() for x in body[max(0, pc - 40):pc] if INSTR.match(x.strip())][-5:]
            print(f"  [{k:2d}] {d}  line {start + pc + 1}  {t.split(';')[0].strip():40s} <- " + ' | '.join(c.split(';')[0].strip() for c in ctx))
        if d == 'T':
            pc = labels[mc.group(1)]
            continue
    pc += 1

print(name[:110])
print(f"  decisions {used}   loop lines {start + loop[0] + 1}..{start + loop[1] + 1}, counted once (x {trips} on the path)")
hdr = ''.join(f"{c:>10s}" for c in CLASSES)
print(f"  {'part':22s}{'slots':>7s}{'no compute':>12s}{hdr}")
tot = tot_idle = 0
for ph in ('prologue', 'loop', 'epilogue'):
    c = counts[ph]
    n, idle = sum(c.values()), sum(c[x] for x in IDLE)
    mult = trips if ph == 'loop' else 1
    tot += n * mult
    tot_idle += idle * mult
    print(f"  {ph:22s}{n:7d}{idle:12d}" + ''.join(f"{c[x]:10d}" for x in CLASSES))
outside = {x: counts['prologue'][x] + counts['epilogue'][x] for x in CLASSES}
n, idle = sum(outside.values()), sum(outside[x] for x in IDLE)
print(f"  {'outside the loop':22s}{n:7d}{idle:12d}" + ''.join(f"{outside[x]:10d}" for x in CLASSES))
print(f"  {'whole path':22s}{tot:7d}{tot_idle:12d}   ({trips} trips)   {tot * 4.1 / 2400:.2f} us at 4.1 cycles per slot and 2.4 GHz")
