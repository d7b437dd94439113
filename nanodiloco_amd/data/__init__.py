"""Data sources: synthetic on-device tokens, native memmap shards, HF datasets (reference path)."""
from .synthetic import SyntheticTokens


def build_data(kind: str, *, vocab_size: int, seq_len: int, batch_size: int, seed: int, rank: int,
               world_size: int, device, dataset_path: str = None, tokenizer: str = "huggyllama/llama-7b",
               mask_pad_labels: bool = True):
    if kind == "synthetic":
        return SyntheticTokens(vocab_size, seq_len, batch_size, seed, rank, device)
    if kind == "memmap":
        import glob
        import os

        from .memmap import MemmapTokens
        paths = sorted(glob.glob(os.path.join(dataset_path, "*.bin"))) if os.path.isdir(dataset_path) \
            else sorted(glob.glob(dataset_path))
        if not paths:
            raise FileNotFoundError(f"no token shards at {dataset_path}")
        return MemmapTokens(paths, seq_len, batch_size, vocab_size, seed, rank, world_size, device=device)
    if kind == "hf":
        from .hf import make_hf_loader
        return _DeviceIter(make_hf_loader(dataset_path, tokenizer, seq_len, batch_size, world_size, rank, seed,
                                          mask_pad_labels), device)
    raise ValueError(f"unknown data source {kind}")


class EvalStream:
    """A held-out stream: ``reset()`` rewinds it, after which it yields the same batches every time."""

    def __init__(self, source, rewind):
        self.source, self._rewind = source, rewind

    def reset(self):
        self._rewind(self.source)
        return self

    def __iter__(self):
        return self

    def __next__(self):
        return next(self.source)


def _shard_paths(dataset_path: str):
    import glob
    import os
    return sorted(glob.glob(os.path.join(dataset_path, "*.bin"))) if os.path.isdir(dataset_path) \
        else sorted(glob.glob(dataset_path))


def build_eval_data(kind: str, *, vocab_size: int, seq_len: int, batch_size: int, seed: int, rank: int,
                    world_size: int, device, eval_dataset_path: str = None) -> EvalStream:
    """The held-out stream of ``--eval-every`` (Trainer.evaluate), apart from the training stream.

    synthetic: a ``SyntheticTokens`` on ``rank_seed(seed, rank, 2)`` (the training stream is stream 1);
    ``reset()`` re-seeds its generator.  memmap: the shards of ``eval_dataset_path`` (a directory of ``*.bin`` or a
    glob), unshuffled, each rank its own windows; ``reset()`` rewinds the cursor.  The training shards are never
    used: without ``eval_dataset_path`` this raises."""
    if kind == "synthetic":
        from ..utils.seed import rank_seed
        src = SyntheticTokens(vocab_size, seq_len, batch_size, seed, rank, device)
        eval_seed = rank_seed(seed, rank, 2)

        def rewind(d):
            d.gen.manual_seed(eval_seed)
            d.samples_drawn = 0

        return EvalStream(src, rewind).reset()
    if kind == "memmap":
        if not eval_dataset_path:
            raise ValueError("--eval-every with --data memmap needs --eval-dataset-path (held-out token shards); "
                             "the training shards are never evaluated on")
        from .memmap import MemmapTokens
        paths = _shard_paths(eval_dataset_path)
        if not paths:
            raise FileNotFoundError(f"no token shards at {eval_dataset_path}")
        src = MemmapTokens(paths, seq_len, batch_size, vocab_size, seed, rank, world_size, shuffle=False,
                           device=device)
        return EvalStream(src, lambda d: d.load_state_dict({"cursor": 0, "base": 0, "world": world_size}))
    if kind == "hf":
        raise NotImplementedError("--eval-every is not supported yet with --data hf (use --data memmap with "
                                  "pre-tokenised held-out shards, scripts/pretokenize.py)")
    raise ValueError(f"unknown data source {kind}")


class _DeviceIter:
    """Moves host batches to the device; forwards the loader's resumable cursor."""

    def __init__(self, loader, device):
        self.loader, self.device = loader, device

    def __iter__(self):
        return self

    def __next__(self):
        b = next(self.loader)
        return {k: v.to(self.device, non_blocking=True) for k, v in b.items()}

    def state_dict(self):
        return self.loader.state_dict()

    def load_state_dict(self, d, resized: bool = False):
        if resized:
            # HFBatches: each rank reads a CONTIGUOUS shard of the dataset (split_dataset_by_node, the
            # reference's sharding); another worker count re-cuts every shard, so no cursor maps onto the
            # new layout without repeating or skipping examples
            raise RuntimeError("--elastic-resume with --data hf cannot keep the data stream exact (the contiguous "
                               "per-rank shards move with the worker count); use --data memmap (pre-tokenised "
                               "shards, scripts/pretokenize.py), whose global stream resumes exactly on any count")
        self.loader.load_state_dict(d)


__all__ = ["SyntheticTokens", "build_data", "build_eval_data", "EvalStream"]
