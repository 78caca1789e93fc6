"""How qpb.h's entry points issue their work: the `stream` argument, the
per-(device, stream) workspace cache (csrc/qpb_workspace.hip) and its two
release calls.

Every case compares the outputs of calls queued on side streams, bitwise and
array by array, with "solo": release_workspaces(), the same call on the current
stream, torch.cuda.synchronize().  (qpb.h: a QP's outputs depend on its own
inputs only, so this holds for the Gram class too, whatever grid walks it.)

The stream pattern (_queue): on a side stream s, with no host sync inside,
  1. a device delay, torch.cuda._sleep(cycles);  2. an event `gate` after it;
  3. the tensors the call reads, NaN until then, receive their values;
  4. every output tensor is filled with the byte 0xA5;  5. the qpb call on s;
  6. ok = not gate.query();  7. s.synchronize().
A kernel, memset or second launch issued on any other stream runs while s still
sleeps: it reads NaN, or the fill of step 4 overwrites what it wrote.  (torch's
pool streams are non-blocking: the null stream does not wait for them.)  `ok`
is the condition of validity, asserted: the delay was still running when the
last call had been queued.

Measured on an MI355X (gfx950): torch.cuda._sleep(1_000_000) lasts 0.4165 ms
by events (41.65 ms for 100 M cycles; SLEEP_MS_PER_MCYCLE), and queueing steps
3-5 takes the host 0.166 ms for the slowest single form, qpb_solve_sections'
Gram build (0.03 to 0.14 ms for the others; HOST_QUEUE_MS_SLOWEST).  CYCLES =
50 M is a delay of 20.8 ms: 125 times that, where at least 20 times is
wanted, and below 200 ms.  The cases that queue several calls (0.40 ms for the
six back-to-back launches, 0.24 ms per stream for two streams) use
CYCLES_MANY = 100 M, 41.7 ms.
"""
import ctypes
import threading
import time

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from test_gpu_status_contract import BOX_N, DENSE, _dev, _same  # noqa: E402

FILL = 0xA5
FLAG_DIAG_NO_REDO = 64
SLEEP_MS_PER_MCYCLE = 0.4165  # measured, see the module docstring
HOST_QUEUE_MS_SLOWEST = 0.166
CYCLES = 50_000_000
CYCLES_MANY = 100_000_000
MAX_DELAY_MS = 200.0

F64, I32, I64 = torch.float64, torch.int32, torch.int64


@pytest.fixture(scope="module")
def qpb():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import qpb as q
    yield q
    _JOBS.clear()  # the shared device inputs and solo results
    q.release_workspaces()


def _route(name):
    return next(r for r in DENSE if r[0] == name)


# --------------------------------------------------------------------- the calls
class Job:
    """One qpb call: its inputs (staging: the values; live: what the call reads,
    NaN until step 3), the shapes of its outputs, and the call itself,
    call(qpb, inputs, outputs, stream) with stream None = the current one."""

    def __init__(self, name, staging, out_specs, call, n_scratch=0):
        self.name, self.staging, self.out_specs, self.call = name, staging, out_specs, call
        self.n_scratch = n_scratch  # trailing outputs that are zeroed, not filled, and not compared (tick counters)
        self.live = [torch.full_like(t, float("nan")) for t in staging]
        self.outs = self.new_outs()
        self.solo = None

    def new_outs(self):
        return [torch.empty(shape, dtype=dt, device="cuda") for shape, dt in self.out_specs]

    def compared(self, outs):
        return outs[:len(outs) - self.n_scratch] if self.n_scratch else outs

    def prefill(self, outs):
        for o in self.compared(outs):
            o.view(torch.uint8).fill_(FILL)
        for o in outs[len(outs) - self.n_scratch:] if self.n_scratch else ():
            o.zero_()


def _sol_specs(B, n, m):
    return [((B, n), F64), ((B, m), F64), ((B, (m + 31) // 32), I32), ((B,), I32), ((B,), I32)]


def _sp(qpb, stream):
    return qpb._stream_ptr(stream)


def _rc(qpb, rc, what):
    assert rc == 0, (what, rc, qpb.lib().qpb_last_error())


def solve_job(name, n, m, B, flags, seed):
    import oracle as O
    H, f, A, b = O.family_conditioned(seed, B, n, m=m, box=10.0, kind="dense")
    return Job(name, _dev(H, f, A, b), _sol_specs(B, n, m),
               lambda q, i, o, s: q.solve(*i, flags=flags, out=q.Solution(*o), stream=s))


def box_job(n, B, seed):
    import oracle as O
    H, f, _, _ = O.family_conditioned(seed, B, n, box=10.0)
    lb, ub = np.full((B, n), -10.0), np.full((B, n), 10.0)
    return Job(f"solve_box-n{n}", _dev(H, f, lb, ub), _sol_specs(B, n, 2 * n),
               lambda q, i, o, s: q.solve_box(*i, out=q.Solution(*o), stream=s))


def _ref_inputs(n, B, seed):
    import oracle as O
    P, q, _, _ = O.family_conditioned(seed, B, n, box=10.0)
    x0 = np.random.default_rng([seed, 5]).uniform(-1e3, 1e3, (B, n))
    return P, q, x0


def ref_job(n, B, seed, iterations=3):
    P, q, x0 = _ref_inputs(n, B, seed)

    def call(qp, i, o, s):
        d = qp.RefDesc(n, qp.REF_NEWTON, B, iterations, 0, -1e12, 1e12)
        _rc(qp, qp.lib().qpb_ref_solve(ctypes.byref(d), *[qp._ptr(t) for t in i + o], _sp(qp, s)), "qpb_ref_solve")

    return Job(f"ref_solve-n{n}", _dev(P, q, x0), [((B, n), F64), ((B,), I32)], call)


def invert_job(n, B, seed):
    P, _, _ = _ref_inputs(n, B, seed)

    def call(qp, i, o, s):
        _rc(qp, qp.lib().qpb_matrix_invert(n, B, qp._ptr(i[0]), qp._ptr(o[0]), _sp(qp, s)), "qpb_matrix_invert")

    return Job(f"matrix_invert-n{n}", _dev(P), [((B, n, n), F64)], call)


def qf_job(n, B, seed):
    P, q, x = _ref_inputs(n, B, seed)

    def call(qp, i, o, s):
        _rc(qp, qp.lib().qpb_qf_eval(n, B, qp._ptr(i[0]), qp._ptr(i[1]), -3.5, qp._ptr(i[2]), qp._ptr(o[0]),
                                     _sp(qp, s)), "qpb_qf_eval")

    return Job(f"qf_eval-n{n}", _dev(P, q, x), [((B,), F64)], call)


def generate_job(n, m, B, family, seed):
    def call(qp, i, o, s):
        d = qp.GenDesc(n, m, B, 3, seed, qp.FAMILIES[family], 0, 1.0, 10.0)
        _rc(qp, qp.lib().qpb_generate(ctypes.byref(d), *[qp._ptr(t) for t in o], _sp(qp, s)), "qpb_generate")

    return Job(f"generate-n{n}-{family}", [], [((B, n, n), F64), ((B, n), F64), ((B, m, n), F64), ((B, m), F64)], call)


def ref_generate_job(n, B, seed):
    def call(qp, i, o, s):
        d = qp.RefGenDesc(n, seed, B, 2, -1e3, 1e3, -1e3, 1e3, -1e3, 1e3)
        _rc(qp, qp.lib().qpb_ref_generate(ctypes.byref(d), *[qp._ptr(t) for t in o], _sp(qp, s)), "qpb_ref_generate")

    return Job(f"ref_generate-n{n}", [], [((B, n, n), F64), ((B, n), F64), ((B, n), F64)], call)


def sections_job(name, n, m, B, seed):
    """qpb_solve_sections: the five outputs are compared; the tick counters are
    zeroed in step 4 and must have been added to after that."""
    import oracle as O
    H, f, A, b = O.family_conditioned(seed, B, n, m=m, box=10.0, kind="dense")

    def call(qp, i, o, s):
        d = qp.Desc(n, m, B, 0, 0, 0.0)
        rows = o[5]
        _rc(qp, qp.lib().qpb_solve_sections(ctypes.byref(d), *[qp._ptr(t) for t in i + o[:5]], qp._ptr(rows),
                                            rows.numel(), _sp(qp, s)), "qpb_solve_sections")

    return Job(name, _dev(H, f, A, b), _sol_specs(B, n, m) + [((256 * 20,), I64)], call, n_scratch=1)


def mixed_job():
    """gi_mixed, 20 x 33.  The even QPs are family_conditioned's (settled by
    the fp32 pass and its refinement); the odd ones have an H of condition
    1e10, beyond an fp32 factorisation, and QP 2 has -H: whatever the fp32
    pass does not end with QPB_OK and verify is left to the fp64 re-solve, the
    second launch."""
    import oracle as O
    name, n, m, B, flags = _route("gi_mixed")
    H, f, A, b = O.family_conditioned(4100, B, n, m=m, box=10.0, kind="dense")
    rs = np.random.default_rng(4101)
    for i in range(1, B, 2):
        Q, _ = np.linalg.qr(rs.standard_normal((n, n)))
        Hi = (Q * (1e3 * 10.0 ** np.linspace(0.0, -10.0, n))) @ Q.T
        H[i] = 0.5 * (Hi + Hi.T)
    H[2] = -H[2]
    return Job(name, _dev(H, f, A, b), _sol_specs(B, n, m),
               lambda q, i, o, s: q.solve(*i, flags=flags, out=q.Solution(*o), stream=s))


GRAM = (48, 96)
_JOBS = {}


def _job(key, make):
    """Jobs (device inputs included) are built once per session and shared."""
    if key not in _JOBS:
        _JOBS[key] = make()
    return _JOBS[key]


def _gram_job(B, seed, n=GRAM[0], m=GRAM[1]):
    return _job(("gram", n, m, B, seed), lambda: solve_job(f"gi_gram-{n}x{m}-B{B}-s{seed}", n, m, B, 0, seed))


def _form_jobs():
    forms = {}

    def add(key, make):
        forms[key] = make

    for rname in ("gi_dense-full", "gi_wave-20x33", "gi_gram-48x96"):
        name, n, m, B, flags = _route(rname)
        add(rname, lambda name=name, n=n, m=m, B=B, flags=flags: solve_job(name, n, m, B, flags, 4000 + n + m))
    add("gi_mixed", mixed_job)
    for n in (7, 20, 40):
        assert n in BOX_N
        add(f"solve_box-n{n}", lambda n=n: box_job(n, 13, 4200 + n))
    for n in (32, 100, 130):  # the LDS, big and huge layouts of qpb_ref.hip
        add(f"ref_solve-n{n}", lambda n=n: ref_job(n, 3, 4300 + n))
        add(f"matrix_invert-n{n}", lambda n=n: invert_job(n, 3, 4400 + n))
    add("qf_eval", lambda: qf_job(16, 257, 4500))
    add("generate-n16-box", lambda: generate_job(16, 32, 37, "box", 4600))
    add("generate-n40-dense", lambda: generate_job(40, 80, 6, "dense", 4601))
    add("ref_generate-n16", lambda: ref_generate_job(16, 37, 4700))
    add("sections-n16", lambda: sections_job("sections-n16", 16, 32, 37, 4800))
    add("sections-wave", lambda: sections_job("sections-wave", 20, 33, 13, 4801))
    add("sections-gram", lambda: sections_job("sections-gram", 48, 96, 6, 4802))
    return forms


FORMS = _form_jobs()


# ------------------------------------------------------------------ the pattern
def _solo(qpb, job):
    """release_workspaces(), the call on the current stream, synchronize;
    computed once per job and left unchanged."""
    if job.solo is None:
        qpb.release_workspaces()
        outs = job.new_outs()
        job.prefill(outs)
        job.call(qpb, job.staging, outs, None)
        torch.cuda.synchronize()
        job.solo = [t.cpu().numpy() for t in job.compared(outs)]
    return job.solo


def _arm(jobs):
    """Before the pattern: the tensors the calls will read hold NaN."""
    for j in jobs:
        for t in j.live:
            t.fill_(float("nan"))
    torch.cuda.synchronize()


def _queue(qpb, s, jobs, cycles):
    """Steps 1-5 for `jobs` on stream s, no host sync; returns the gate event
    and the host time (ms) of steps 3-5."""
    with torch.cuda.stream(s):
        torch.cuda._sleep(cycles)
        gate = torch.cuda.Event()
        gate.record()
        t0 = time.perf_counter()
        for j in jobs:
            for live, st in zip(j.live, j.staging):
                live.copy_(st)
            j.prefill(j.outs)
    for j in jobs:
        j.call(qpb, j.live, j.outs, s)
    return gate, (time.perf_counter() - t0) * 1e3


def _surviving(arrays):
    """Elements that still hold the fill pattern, per array."""
    left = []
    for a in arrays:
        raw = np.ascontiguousarray(a).view(np.uint8).reshape(-1, a.dtype.itemsize)
        left.append(int((raw == FILL).all(axis=1).sum()))
    return left


def _check(qpb, job, what=""):
    """After the stream was synchronised: no fill survives, equal to solo."""
    got = [t.cpu().numpy() for t in job.compared(job.outs)]
    want = _solo(qpb, job)
    assert _surviving(got) == [0] * len(got), (what, job.name, "elements never written", _surviving(got))
    assert _same(got, want), (what, job.name, [int((g != w).sum()) for g, w in zip(got, want)])
    if job.n_scratch:
        assert int(job.outs[-1].sum()) > 0, (what, job.name, "no ticks added after the counters were zeroed")


def _run(qpb, plan, cycles, what):
    """plan: [(stream, [jobs])]; every stream behind its own delay, all of them
    queued before any is synchronised."""
    jobs = [j for _, js in plan for j in js]
    assert len({id(j) for j in jobs}) == len(jobs)
    for j in jobs:
        _solo(qpb, j)
    _arm(jobs)
    queued = [_queue(qpb, s, js, cycles) for s, js in plan]
    ok = all(not gate.query() for gate, _ in queued)
    for s, _ in plan:
        s.synchronize()
    print(f"{what}: host queueing " + ", ".join(f"{ms:.3f} ms" for _, ms in queued))
    assert ok, f"{what}: delay too short ({cycles} cycles): the case proved nothing"
    for j in jobs:
        _check(qpb, j, what)


# ------------------------------------------------------- the delay, measured once
def test_delay_is_long_enough_and_bounded(qpb):
    """torch.cuda._sleep by events: CYCLES_MANY stays within 200 ms, and the
    figures in the module docstring are printed again."""
    s = torch.cuda.Stream()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(s):
        torch.cuda._sleep(1000)  # the kernel's first launch
        e0.record()
        torch.cuda._sleep(CYCLES_MANY)
        e1.record()
    s.synchronize()
    ms = e0.elapsed_time(e1)
    print(f"_sleep({CYCLES_MANY}) = {ms:.2f} ms: {ms / CYCLES_MANY * 1e6:.4f} ms per 1e6 cycles; "
          f"CYCLES = {ms * CYCLES / CYCLES_MANY:.2f} ms")
    assert ms <= MAX_DELAY_MS, ms
    assert ms * CYCLES / CYCLES_MANY >= 20 * HOST_QUEUE_MS_SLOWEST, (ms, HOST_QUEUE_MS_SLOWEST)


# ------------------------------------------- a. every entry point, on its stream
@pytest.mark.parametrize("form", list(FORMS))
def test_runs_on_the_given_stream(qpb, form):
    """Steps 1-7 of the module docstring for one call of every entry point and
    kernel form: equal to solo."""
    job = _job(("form", form), FORMS[form])
    if form == "gi_mixed":
        # validity: the batch takes both launches (some QPs are left to the fp64 re-solve, not all)
        name, n, m, B, flags = _route("gi_mixed")
        st = qpb.solve(*job.staging, flags=flags | FLAG_DIAG_NO_REDO).status.cpu().numpy()
        print(f"gi_mixed: {int((st == qpb.STATUS_REDO).sum())} of {B} QPs left to the re-solve")
        assert 0 < (st == qpb.STATUS_REDO).sum() < B, st
    _run(qpb, [(torch.cuda.Stream(), [job])], CYCLES, form)


# ------------------------------- b. back-to-back workspace launches on one stream
def _tenants():
    """The cached buffer's tenants in turn: the Gram kernel with a small and a
    large grid (300 QPs: more than CUs, so the queue is walked, and the buffer
    grows while the launch before is still queued), the reference replicas'
    big and huge layouts, the Gram kernel's BOX form, the Gram kernel again."""
    return [_gram_job(5, 5001), _gram_job(300, 5002),
            _job(("ref", 100, 300), lambda: ref_job(100, 300, 5003)),
            _job(("ref", 130, 4), lambda: ref_job(130, 4, 5004)),
            _job(("box", 64, 270), lambda: box_job(64, 270, 5005)),
            _gram_job(5, 5006, 33, 40)]


def test_back_to_back_workspace_launches(qpb):
    """Six launches that share one cached buffer, queued on one side stream
    behind the delay with no sync between them: each equal to its solo result,
    no fill pattern left (a stale queue head, a memset on another stream or a
    buffer freed under a queued launch leaves QPs unwritten)."""
    _run(qpb, [(torch.cuda.Stream(), _tenants())], CYCLES_MANY, "back to back")


# ------------------------------------------------------------ c. two streams at once
def _two_stream_plan(s1, s2):
    on1 = [_gram_job(300, 5100 + k) for k in range(3)]
    on2 = [_gram_job(300, 5103), _job(("ref", 100, 300, "c"), lambda: ref_job(100, 300, 5104)), _gram_job(300, 5105)]
    return [(s1, on1), (s2, on2)]


@pytest.mark.parametrize("second", ["side", "default"])
def test_two_streams_at_once(qpb, second):
    """Three Gram solves on one side stream; two with a reference solve between
    them on a second side stream, or on the default stream.  Both are queued
    in full, each behind its own delay, before either runs: the streams'
    buffers and queue heads are independent, all equal to solo."""
    s2 = torch.cuda.Stream() if second == "side" else torch.cuda.default_stream()
    _run(qpb, _two_stream_plan(torch.cuda.Stream(), s2), CYCLES_MANY, f"two streams ({second})")


# ------------------------------------------------------------- d. release semantics
def test_release_semantics(qpb):
    job = _gram_job(300, 5002)
    want = _solo(qpb, job)
    s = torch.cuda.Stream()
    _arm([job])
    gate, _ = _queue(qpb, s, [job], CYCLES)
    after = torch.cuda.Event()
    after.record(s)
    ok = not gate.query()
    qpb.release_stream_workspace(s)  # frees stream-ordered and waits: the queued work is done
    assert after.query(), "release_stream_workspace returned before the work queued on the stream had finished"
    assert ok, "delay too short: the case proved nothing"
    got = [t.cpu().numpy() for t in job.outs]
    assert _surviving(got) == [0] * 5 and _same(got, want)
    # the stream is usable afterwards
    _run(qpb, [(s, [job])], CYCLES, "after release_stream_workspace")
    # a stream that was never used, and everything twice in a row
    qpb.release_stream_workspace(torch.cuda.Stream())
    qpb.release_workspaces()
    qpb.release_workspaces()
    # the default stream after release_workspaces()
    job.prefill(job.outs)
    job.call(qpb, job.staging, job.outs, None)
    torch.cuda.synchronize()
    assert _same([t.cpu().numpy() for t in job.outs], want)
    qpb.release_stream_workspace(None)
    qpb.release_stream_workspace(None)


# ------------------------------------------------------------------ e. host threads
def test_host_threads_share_a_stream(qpb):
    """qpb.h: "a buffer is handed to a launch only while the cache is locked".
    Two host threads share one side stream (ctypes drops the GIL during the
    call), each with 8 Gram solves into its own outputs, alternating B = 5
    (small grid) and B = 300 (the buffer grows); a third thread releases that
    stream's buffer four times.  Bounded, runs once."""
    small, large = _gram_job(5, 5001), _gram_job(300, 5002)
    want = {id(small): _solo(qpb, small), id(large): _solo(qpb, large)}
    s = torch.cuda.Stream()
    qpb.release_workspaces()
    seq = [small, large] * 4
    outs = [[j.new_outs() for j in seq] for _ in range(2)]
    for per_thread in outs:
        for j, o in zip(seq, per_thread):
            j.prefill(o)
    torch.cuda.synchronize()
    errors = []

    def solver(t):
        try:
            for j, o in zip(seq, outs[t]):
                j.call(qpb, j.staging, o, s)
        except Exception as e:  # noqa: BLE001
            errors.append(e)

    def releaser():
        try:
            for _ in range(4):
                qpb.release_stream_workspace(s)
        except Exception as e:  # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=solver, args=(0,)), threading.Thread(target=solver, args=(1,)),
               threading.Thread(target=releaser)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    s.synchronize()
    assert not errors, errors
    for t in range(2):
        for k, (j, o) in enumerate(zip(seq, outs[t])):
            got = [a.cpu().numpy() for a in o]
            assert _surviving(got) == [0] * 5, (t, k, j.name, _surviving(got))
            assert _same(got, want[id(j)]), (t, k, j.name)
    qpb.release_stream_workspace(s)
