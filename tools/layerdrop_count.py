"""Dropped transformer-layer instances of bench.py's timed steps, counted on the host from the staged LayerDrop keep flags.

    python tools/layerdrop_count.py [--steps 100] [--warmup 5]        (one line of JSON on stderr, bench.py's own line on stdout)

Runs bench.py's main() unchanged with functional.stage_host wrapped: every staged producer that returns a LayerDrop flag vector (float32,
one 0 / 1 entry per layer of a stack) is counted per call.  An update stages four of them (encoder + decoder of the speech and of the text
micro-batch: 36 layer instances for Base); the producers run once per eager / recorded update and once before every replay, so the timed
steps are the flag sets [warmup, warmup + steps) (a prefetched set for the step after the last one is ignored)."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import torch
    import bench
    from speecht5_amd import functional as Fn
    steps = int(sys.argv[sys.argv.index("--steps") + 1]) if "--steps" in sys.argv else 100
    warmup = int(sys.argv[sys.argv.index("--warmup") + 1]) if "--warmup" in sys.argv else 5
    sets = []       # one entry per produced flag vector: (layers, dropped)
    stacks = (12, 6)        # layers of the Base encoder / decoder: the only staged 0 / 1 float vectors of these lengths
    real = Fn.stage_host

    def stage_host(producer, device):
        def counted():
            h = producer()
            if torch.is_tensor(h) and h.dtype == torch.float32 and h.dim() == 1 and h.numel() in stacks and bool(((h == 0) | (h == 1)).all()):
                sets.append((h.numel(), int((h == 0).sum())))
            return h
        return real(counted, device)

    Fn.stage_host = stage_host
    sys.argv = [sys.argv[0], "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup), "--no-cpu-baseline"]
    bench.main()
    per_update = 4
    assert len(sets) >= (warmup + steps) * per_update, (len(sets), warmup, steps)
    timed = sets[warmup * per_update:(warmup + steps) * per_update]
    layers = sum(n for n, _ in timed)
    dropped = sum(d for _, d in timed)
    per_step = [sum(d for _, d in timed[i * per_update:(i + 1) * per_update]) for i in range(steps)]
    print(json.dumps({"timed_steps": steps, "layer_instances": layers, "dropped_instances": dropped,
                      "dropped_per_update": round(dropped / steps, 3), "max_in_one_update": max(per_step),
                      "updates_without_a_drop": sum(1 for v in per_step if v == 0),
                      "dropped_by_stack_position": {"speech_enc": sum(d for _, d in timed[0::4]), "speech_dec": sum(d for _, d in timed[1::4]),
                                                    "text_enc": sum(d for _, d in timed[2::4]), "text_dec": sum(d for _, d in timed[3::4])}}),
          file=sys.stderr)


if __name__ == "__main__":
    main()
