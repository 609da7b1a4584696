"""Static view of the tile hand-over of one kernel in an asm file: isa_tile_tail.py file.s kernel_substring

Walks the control flow from the tile loop's last barrier (the last s_barrier in the text: nothing after the loop has
one) through the loop-top barrier to the barrier that ends the first phase of the next tile, every branch both ways,
and lists what a wave can meet there of: vector-memory loads, scratch accesses, s_waitcnt vmcnt(...),
stores and atomics.  "tail" = before the loop-top barrier, "head" = after it.  The exit path after the last tile is
walked to s_endpgm and shown as "exit".  The walk must meet exactly two distinct barriers (loop top, end of the first
phase), else the kernel is not laid out as assumed and the tool stops with an error.
"""
import re
import sys

path, key = sys.argv[1], sys.argv[2]
lines = open(path).read().split('\n')
start = next(i for i, l in enumerate(lines) if l.startswith('_ZN') and key in l and ':' in l)
end = next(i for i in range(start, len(lines)) if lines[i].strip().startswith('.Lfunc_end'))
label = {}
for i in range(start, end):
    m = re.match(r'(\.LBB\w+):', lines[i])
    if m:
        label[m.group(1)] = i


def op_of(i):
    l = lines[i].strip()
    return l.split()[0] if l and not l.startswith((';', '.')) else None


barriers = [i for i in range(start, end) if op_of(i) == 's_barrier']
seen, todo = {}, [(barriers[-1] + 1, 0)]          # line -> fewest barriers passed on the way there
while todo:
    i, nb = todo.pop()
    while i < end and (i not in seen or seen[i] > nb):
        seen[i] = nb
        op = op_of(i)
        if op == 's_barrier':
            nb += 1
            if nb == 2:
                break
        elif op == 's_endpgm':
            break
        elif op and op.startswith(('s_branch', 's_cbranch')):
            todo.append((label[lines[i].split()[-1]], nb))
            if op == 's_branch':
                break
        i += 1
met = sorted(i for i in seen if op_of(i) == 's_barrier')
if len(met) != 2 or {seen[i] for i in met} != {0, 1}:
    sys.exit("%s: the walk from the last s_barrier met %d barriers, expected loop top + end of the first phase" % (key, len(met)))


def successors(i):
    op = op_of(i)
    if op in ('s_endpgm', 's_barrier'):
        return []
    if op and op.startswith(('s_branch', 's_cbranch')):
        return [label[lines[i].split()[-1]]] + ([] if op == 's_branch' else [i + 1])
    return [i + 1]


loops = {i for i in seen if op_of(i) == 's_barrier'}          # lines from which a barrier is reached: inside the loop
grew = True
while grew:
    grew = False
    for i in seen:
        if i not in loops and any(n in loops for n in successors(i)):
            loops.add(i)
            grew = True
exit_only = set(seen) - loops
kinds = {'load': 0, 'scratch': 0, 'vmcnt': 0, 'store': 0}
print("%s: %d s_barrier in the kernel; tile tail from line %d" % (key, len(barriers), barriers[-1] + 1))
for i in sorted(seen, key=lambda i: (i < barriers[-1], i)):      # program order: the tail's first block sits last in the text
    op, l = op_of(i), lines[i].strip()
    if not op:
        continue
    where = 'exit' if i in exit_only else ('tail' if seen[i] == 0 else 'head')
    kind = None
    if op == 's_barrier':
        print("%6d  %-4s ---- s_barrier (%s)" % (i + 1, where, 'loop top' if seen[i] == 0 else 'end of the first phase'))
    elif op.startswith('scratch_'):
        kind = 'scratch'
    elif op.startswith(('buffer_', 'global_', 'flat_')):
        kind = 'store' if re.match(r'(buffer|global|flat)_(store|atomic)', op) else 'load'
    elif op == 's_waitcnt' and 'vmcnt' in l:
        kind = 'vmcnt'
    if kind:
        if where != 'exit':
            kinds[kind] += 1
        print("%6d  %-4s %-7s %s" % (i + 1, where, kind, re.sub(r'\s+', ' ', l)))
print("between the last barrier and the end of the first phase: %d loads, %d scratch accesses, %d vmcnt waits, %d stores" % (
    kinds['load'], kinds['scratch'], kinds['vmcnt'], kinds['store']))
