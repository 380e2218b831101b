"""A model of the two-phase schedule of the block-3 entry kernel (entry_block.hip config 21) over the
host's step plan: which ring slots, A buffers and carried registers every part of an iteration reads
and writes, with the kernel's own slot rules. No GPU.

Iteration ``it`` of a workgroup (it = first step - 1 .. last step) runs, between two barriers each,

    DW phase    dw2(it): y1 ring -> A2      dw1(it + 1): x ring -> A1, + the residual of pooled row k + 1
    GEMM phase  GEMM2(it): A2 -> output     GEMM1(it + 1): A1 -> y1 ring;   the x-row DMA of step it + 2

Everything in one phase runs concurrently (eight waves, no order between them), so within a phase no
location may be both written and read, or written twice; a read must find the value its step expects,
which fails if anything overwrote it before its last read. The residual is computed two iterations
ahead of the output that adds it and is carried in registers; every output must consume the residual
of its own pooled row, also where one workgroup walks several runs back to back."""
import pytest

from kdl.ops.entry_block import OUT, WARM_Y1, plan_steps

PC = 13                   # pooled columns per strip (config 21)


def xslot(row):
    """x ring slot of an input row (entry_block.hip dma_rows / dw1)."""
    return row & 3


def yslot(j, o):
    """y1 ring slot of row R + o (o = 0..3) of step j: counted by steps (step j writes its rows R+2, R+3
    into pair j & 1 and reads R, R+1 from its predecessor's pair)."""
    return 2 * ((j + (o >> 1) + 1) & 1) + (o & 1)


class Phase:
    """Reads and writes of one barrier interval; writes become visible at its end."""

    def __init__(self, state, name):
        self.state, self.name, self.reads, self.writes = state, name, set(), {}

    def read(self, loc, want):
        assert loc not in self.writes, f"{self.name}: {loc} read and written in one phase"
        self.reads.add(loc)
        assert self.state.get(loc) == want, f"{self.name}: {loc} holds {self.state.get(loc)}, step wants {want}"

    def write(self, loc, val):
        assert loc not in self.reads, f"{self.name}: {loc} written and read in one phase"
        assert loc not in self.writes, f"{self.name}: {loc} written twice in one phase"
        self.writes[loc] = val

    def close(self):
        self.state.update(self.writes)


def dma_rows(ph, step):
    """The x rows a step's DMA brings: all four of a run's first step, else the two new ones."""
    b, s, k, mode = step
    R = 2 * k
    for row in (range(R + 1, R + 5) if mode == WARM_Y1 else range(R + 3, R + 5)):
        ph.write(("x", xslot(row)), (b, s, row))


def walk(steps, s0, s1, carry_depth=2, dma_early=False):
    """One workgroup's iterations; returns the outputs it produced as (b, s, k). ``carry_depth`` and
    ``dma_early`` are there to break the schedule on purpose (last test): the kernel's are 2 and False."""
    state, outs = {}, []
    res = [None, None, None]          # residual carry: of the output of step it, it + 1, it + 2
    carry = None                      # y2 row R + 2 of the previous step
    pro = Phase(state, "prologue")
    dma_rows(pro, steps[s0])
    pro.close()
    for it in range(s0 - 1, s1):
        cur = steps[it] if it >= s0 else None
        nxt = steps[it + 1] if it + 1 < s1 else None
        dw = Phase(state, f"DW phase {it}")
        if dma_early and it + 2 < s1:
            dma_rows(dw, steps[it + 2])
        if cur and cur[3] != WARM_Y1:
            b, s, k, _ = cur
            for o in range(4):                                   # y2 rows R+1, R+2 read y1 rows R .. R+3
                dw.read(("y1", yslot(it, o)), (b, s, 2 * k + o))
            dw.write(("A2",), it)
        if nxt:
            b, s, k, mode = nxt
            for row in range(2 * k + 1, 2 * k + 5):              # y1 rows R+2, R+3 read x rows R+1 .. R+4
                dw.read(("x", xslot(row)), (b, s, row))
            dw.write(("A1",), it + 1)
            if mode != WARM_Y1:                                  # residual of pooled row k + 1: x row 2k + 2
                dw.read(("x", xslot(2 * k + 2)), (b, s, 2 * (k + 1)))
                res[2] = (b, s, k + 1)
        dw.close()
        ge = Phase(state, f"GEMM phase {it}")
        if not dma_early and it + 2 < s1:
            dma_rows(ge, steps[it + 2])
        if cur and cur[3] != WARM_Y1:
            b, s, k, mode = cur
            ge.read(("A2",), it)
            if mode == OUT:
                assert carry == (b, s, 2 * k), f"step {it}: carried y2 row {carry}, wants {(b, s, 2 * k)}"
                assert res[0] == (b, s, k), f"step {it}: output {(b, s, k)} adds the residual of {res[0]}"
                outs.append((b, s, k))
            carry = (b, s, 2 * k + 2)
        if nxt:
            b, s, k, _ = nxt
            ge.read(("A1",), it + 1)
            for o in (2, 3):
                ge.write(("y1", yslot(it + 1, o)), (b, s, 2 * k + o))
        ge.close()
        res = [res[1], res[2], res[2]] if carry_depth == 2 else [res[2], res[2], res[2]]
    return outs


@pytest.mark.parametrize("grid", [1, 2, 3, 7, 256])
@pytest.mark.parametrize("OH,OW", [(3, 3), (5, 15), (15, 5), (16, 28), (37, 37)])
def test_two_phase_schedule_has_no_hazard_and_carries_the_right_residual(OH, OW, grid):
    B = 2
    steps, off = plan_steps(B, OH, OW, PC, grid)
    outs = []
    for s0, s1 in zip(off, off[1:]):
        if s0 < s1:
            outs += walk(steps, s0, s1)
    ns = (OW + PC - 1) // PC
    assert sorted(outs) == [(b, s, k) for b in range(B) for s in range(ns) for k in range(OH)]   # each once


def test_the_model_catches_a_shallow_carry_and_an_early_dma():
    """The checks are live: a residual carried one iteration instead of two, and the x-row DMA of step
    it + 2 issued before barrier A instead of after it, both fail on a plan that passes above."""
    steps, off = plan_steps(2, 16, 28, PC, 1)
    walk(steps, off[0], off[1])
    with pytest.raises(AssertionError, match="adds the residual of"):
        walk(steps, off[0], off[1], carry_depth=1)
    with pytest.raises(AssertionError, match="in one phase"):
        walk(steps, off[0], off[1], dma_early=True)
