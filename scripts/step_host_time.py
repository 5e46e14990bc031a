"""Host time of one `step()` on the replay path, no GPU: python scripts/step_host_time.py [tree]   (default: this tree; a parent
checkout as `tree` measures its `Rollout.step` the same way).  A bare `Rollout` object with the attributes the replay path reads, a
graph whose `replay()` does nothing and a cache that is never stale: what is timed is the bound check, the two comparisons in front
of a replay and the call itself (`timeit`, 1e5 calls, best of 5)."""
import os
import sys
import timeit

tree = os.path.abspath(sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, tree)
from graphs4cfd_amd import ops                      # noqa: E402
from graphs4cfd_amd.nn.rollout import Rollout       # noqa: E402


class Nothing:
    def replay(self):
        pass

    def stale(self):
        return False


ro = Rollout.__new__(Rollout)
ro.max_steps, ro.steps_done, ro.exact_range, ro.capture = 10 ** 9, 2, False, True
ro._epoch, ro._hipgraph, ro.static = ops.weights_epoch(), Nothing(), Nothing()
best = min(timeit.repeat(ro.step, number=100_000, repeat=5)) / 100_000
print(f"{tree}: {type(ro).step.__qualname__} on the replay path: {1e6 * best:.3f} us per call")
