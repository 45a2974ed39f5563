"""CPU: the stream / event protocol of artgpu_batch_run_io (art_amd/csrc/api_batch.hip io_frame) replayed as a discrete-event model.

Per lane: an upload stream, the context's stream and a download stream; two staging slots on each side and two working images, picked by
the parity of the frame's turn.  Every frame carries its own residency -- where its sensor data lies (device / pinned / pageable) and where
its scanlines go (device / pinned, written directly by the download stream's kernel / pinned, staged and copied / pageable) -- and the model
queues exactly the operations, records and waits io_frame queues for that pair, in its order, with HIP's semantics: a stream runs its
operations in order; hipStreamWaitEvent holds the stream back until the record that was the event's latest WHEN THE WAIT WAS QUEUED has
completed, and is a no-op on an event that was never recorded.  Every operation gets a random duration, log-uniform over three and a half
decades (one download has to be able to outlast a whole frame on the context's stream for some of the hazards to show); the three streams
run as early as their dependencies allow, and then every buffer is checked: a reader of turn i sees the bytes of turn i (the writer of turn
i has finished, no later writer has started).  Dropping any one of the protocol's waits makes the check fail, which the last tests show.

Not modelled, because they cannot race: the CFA plane and the flag words (written and read on the context's stream only), and the caller's
own buffers (one per frame)."""
import itertools
import random

import pytest

IN_KINDS = ("device", "pinned", "pageable")
OUT_KINDS = ("device", "pinned-direct", "pinned-staged", "pageable")
FRAME_KINDS = tuple(itertools.product(IN_KINDS, OUT_KINDS))
NEUTRAL = ("pageable", "pageable")                     # everything on the context's stream: takes part in no cross-stream ordering


def simulate(nframes, seed, drop=None, pinned_in=True, pinned_out=True, kinds=None):
    """`kinds`: per frame (input kind, output kind); None: the same residency for the whole batch, from pinned_in / pinned_out (pinned
    scanlines staged and copied: option io_direct = 0).  `drop`: leave one wait of the protocol out -- "scaled", "up", "down", "comp" each
    drop that wait everywhere; "down_before_device" drops the `down` wait only in front of a frame whose scanlines stay on the device, which
    is the condition io_frame had (`i >= 2 && !out->on_device`) before the wait was made unconditional."""
    rng = random.Random(seed)
    if kinds is None:
        kinds = [("pinned" if pinned_in else "pageable", "pinned-staged" if pinned_out else "pageable")] * nframes
    assert len(kinds) == nframes
    tfree = {"U": 0.0, "C": 0.0, "D": 0.0}          # per stream: when its last queued operation ends (a stream runs in program order)
    last_record = {}                                   # event name -> when the record that is the event's latest "now", in host program order, completes
    ops = []

    # Every dependency of an operation -- its predecessor on the stream, the records its stream has waited for -- is queued before it, so
    # the time it starts at is known when it is queued: as early as those allow.  (No deadlock is possible, as in HIP.)
    def op(stream, name, turn, reads=(), writes=()):
        start = tfree[stream]
        o = {"stream": stream, "name": name, "turn": turn, "reads": reads, "writes": writes, "start": start,
             "end": start + 10.0 ** rng.uniform(-2.0, 1.5)}
        tfree[stream] = o["end"]; ops.append(o)
        return o

    def record(stream, ev):                            # hipEventRecord: completes when everything queued on the stream so far has
        last_record[ev] = tfree[stream]

    def wait(stream, ev):                              # hipStreamWaitEvent: the record as of now; never recorded: nothing to wait for
        if ev in last_record:
            tfree[stream] = max(tfree[stream], last_record[ev])

    # (":N" names the line of art_amd/csrc/api_batch.hip, in io_frame, that the operation mirrors; the model has no wait that io_frame lacks)
    for i, (kin, kout) in enumerate(kinds):
        assert kin in IN_KINDS and kout in OUT_KINDS
        s = i & 1
        up = "C" if kin == "pageable" else "U"                          # :192 s_up (a pageable copy stays on the context's stream)
        down = "D" if kout.startswith("pinned") else "C"                # :193 s_down
        direct = kout == "pinned-direct"                                # :195 host_dev
        on_device = kout == "device"
        if i >= 2 and drop != "down" and not (drop == "down_before_device" and on_device):
            wait("C", f"down{s}")                                       # :202 working image / staging-out slot of turn i - 2 downloaded
        if kin != "device":
            if i >= 2 and drop != "scaled":
                wait(up, f"scaled{s}")                                  # :210 the kernel that read this slot two turns ago
            op(up, "h2d", i, writes=[f"in{s}"])                         # :212 hipMemcpy2DAsync into the staging slot
            record(up, f"up{s}")                                        # :213
            if drop != "up":
                wait("C", f"up{s}")                                     # :214
            op("C", "scale_colors", i, reads=[f"in{s}"])                # :221 launch_scale_colors (into the CFA plane)
            record("C", f"scaled{s}")                                   # :222
        else:
            op("C", "scale_colors", i)                                  # :221 reads the caller's device buffer
        op("C", "pipeline", i, writes=[f"img{s}"])                      # :227-246 CA, pipeline_run_impl, rgb2out in place
        if direct:
            record("C", f"comp{s}")                                     # :252
            if drop != "comp":
                wait("D", f"comp{s}")                                   # :253
            op("D", "scanlines_host", i, reads=[f"img{s}"])             # :255 launch_scanlines_host into the caller's pinned buffer
            record("D", f"down{s}")                                     # :256
            continue
        if on_device:
            op("C", "scanlines", i, reads=[f"img{s}"])                  # :265 launch_scanlines into the caller's device buffer
            continue                                                    # (:267 nothing recorded, nothing downloaded)
        op("C", "scanlines", i, reads=[f"img{s}"], writes=[f"out{s}"])  # :265 launch_scanlines into the staging slot
        record("C", f"comp{s}")                                         # :268
        if drop != "comp":
            wait(down, f"comp{s}")                                      # :269
        op(down, "d2h", i, reads=[f"out{s}"])                           # :270 hipMemcpy2DAsync to the caller's buffer
        record(down, f"down{s}")                                        # :271

    return ops


def hazards(ops):
    bad = []
    writers = {}
    for o in ops:
        for b in o["writes"]:
            writers.setdefault(b, []).append(o)
    for o in ops:
        for b in o["reads"]:
            ws = sorted(writers[b], key=lambda w: w["turn"])
            mine = [w for w in ws if w["turn"] == o["turn"]][0]
            if mine["end"] > o["start"] + 1e-12:
                bad.append((o["name"], o["turn"], b, "reads before its writer finished"))
            for later in (w for w in ws if w["turn"] > o["turn"]):
                if later["start"] < o["end"] - 1e-12:
                    bad.append((o["name"], o["turn"], b, f"overwritten by turn {later['turn']} while being read"))
                    break
    return bad


@pytest.mark.parametrize("pinned_in,pinned_out", [(True, True), (False, True), (True, False), (False, False)])
def test_protocol_has_no_hazard(pinned_in, pinned_out):
    for seed in range(200):
        ops = simulate(9, seed, pinned_in=pinned_in, pinned_out=pinned_out)
        assert not hazards(ops), (seed, hazards(ops)[:3])


@pytest.mark.parametrize("kind", FRAME_KINDS, ids=lambda k: "-".join(k) if isinstance(k, tuple) else str(k))
def test_protocol_has_no_hazard_with_one_residency_of_every_kind(kind):
    """the direct download and device buffers, which the four cases above do not have"""
    for seed in range(100):
        ops = simulate(9, seed, kinds=[kind] * 9)
        assert not hazards(ops), (seed, hazards(ops)[:3])


def test_copies_really_overlap_the_kernels():
    """the point of the three streams: in steady state an upload and a download run while the context's stream computes"""
    ops = simulate(12, 3)
    c = [(o["start"], o["end"]) for o in ops if o["stream"] == "C"]
    def overlaps(o):
        return any(s < o["end"] and o["start"] < e for s, e in c)
    assert sum(overlaps(o) for o in ops if o["name"] == "h2d" and o["turn"] >= 2) >= 6
    assert sum(overlaps(o) for o in ops if o["name"] == "d2h" and o["turn"] < 10) >= 6


def _lane(first, second, fillers):
    """seven turns with `first` at turn 2 and `second` at turn 4: the two share staging slot and working image 0"""
    kinds = list(fillers)
    kinds[2], kinds[4] = first, second
    return kinds


@pytest.mark.parametrize("fillers", ["neutral", "random"])
def test_no_pair_of_frame_kinds_two_turns_apart_is_hazardous(fillers):
    """every ordered pair of (input kind, output kind) at turns i - 2 and i of one lane, behind and between frames that take part in no
    ordering (pageable both sides) and behind and between frames of any kind"""
    for first, second in itertools.product(FRAME_KINDS, FRAME_KINDS):
        for seed in range(200):
            pick = random.Random(1000 + seed)
            fill = [NEUTRAL] * 7 if fillers == "neutral" else [pick.choice(FRAME_KINDS) for _ in range(7)]
            kinds = _lane(first, second, fill)
            bad = hazards(simulate(7, seed, kinds=kinds))
            assert not bad, (first, second, seed, kinds, bad[:3])


def test_the_wait_that_was_missing_in_front_of_device_outputs():
    """The record of what was wrong: io_frame used to queue the `down` wait only `if (i >= 2 && !out->on_device)`.  With that condition
    exactly one ordered pair of output kinds is hazardous, whatever the inputs: scanlines that the download stream's kernel writes directly
    from working image s (turn i - 2), then a frame whose scanlines stay on the device (turn i), whose pipeline overwrites image s with
    nothing between it and that kernel.  (A staged download reads the staging slot, which a device-output frame does not write.)"""
    hazardous = set()
    for first, second in itertools.product(FRAME_KINDS, FRAME_KINDS):
        for seed in range(200):
            bad = hazards(simulate(7, seed, drop="down_before_device", kinds=_lane(first, second, [NEUTRAL] * 7)))
            if bad:
                assert all(h[:3] == ("scanlines_host", 2, "img0") and "turn 4" in h[3] for h in bad), (first, second, seed, bad[:3])
                hazardous.add((first, second))
                break
    assert {(a[1], b[1]) for a, b in hazardous} == {("pinned-direct", "device")}
    assert len(hazardous) == len(IN_KINDS) ** 2          # with every pair of input kinds


@pytest.mark.parametrize("drop", ["scaled", "up", "down", "comp"])
def test_every_wait_of_the_protocol_is_needed(drop):
    assert any(hazards(simulate(9, seed, drop=drop)) for seed in range(200)), drop


@pytest.mark.parametrize("drop", ["down", "comp"])
def test_every_wait_of_the_direct_download_is_needed(drop):
    kinds = [("pinned", "pinned-direct")] * 9
    assert any(hazards(simulate(9, seed, drop=drop, kinds=kinds)) for seed in range(200)), drop
