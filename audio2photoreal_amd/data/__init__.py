"""Capture directories (the reference's data_loaders/): host loading in `capture`, GPU batch assembly in `batches`."""
from .capture import Take, chunk_plan, chunk_starts, load_capture, load_wav_normalized, split_indices, test_split  # noqa: F401


def __getattr__(name):
    if name == "CaptureBatches":                # imports torch and, on use, the HIP library
        from .batches import CaptureBatches
        return CaptureBatches
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
