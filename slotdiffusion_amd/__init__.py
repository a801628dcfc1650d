"""MI355X-native SlotDiffusion hot path."""


def configure_runtime(graph_queues=None, warn=True):
    """Kept for callers of earlier versions; changes nothing and returns None.  The package sets no HIP runtime
    variable, neither on import nor here: a captured train step replays on the runtime's default queue pool.  Since
    the data and weight gradients of a layer run as one launch (sdmi_bwd_pair) the step time no longer depends on the
    size of that pool (docs/history/rounds_1-5.md, round 3)."""
    return None
