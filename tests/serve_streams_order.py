"""The load of the ``serve(streams=)`` contract tests: one seeded probe among 23 others on 16 slots and 24 streams, in ONE
submission order that tests/test_serve_streams_cpu.py proves to park the probe twice and to move it to another slot, and that
tests/test_serve_streams_gpu.py then runs on the device.

Fair share at chunk_frames 4, ids in submission order (the probe is id 8): step 1 runs 0..15; step 2 the eight joiners 16..23
and 0..7 - 8..15 are parked; step 3 runs 8..23 (the probe returns, into slot 0); step 4 runs 0..15; step 5 runs 16..23 and 0..7 -
the probe is parked again; step 6 runs 8..23 and the probe, at 12 of its 14 frames, ends there.  Nobody ends before step 5, so
the schedule up to the probe's second park does not depend on what is sampled."""
SLOTS, STREAMS, CHUNK = 16, 24, 4
PROBE_AT = 8                # the probe's place in the submission order (= its request id on a fresh server)
PROBE_FRAMES = 14           # ends inside a chunk of 4
OTHER_FRAMES = 20
OTHERS = STREAMS - 1


def submit_all(submit_probe, submit_other):
    """Submit the 24 requests in the order of the contract: ``submit_other(i)`` for i in 0..22, ``submit_probe()`` after the
    first ``PROBE_AT`` of them.  Returns (probe, others)."""
    others = [submit_other(i) for i in range(PROBE_AT)]
    probe = submit_probe()
    others += [submit_other(i) for i in range(PROBE_AT, OTHERS)]
    return probe, others
