"""Training on the MI355X: the reference's train/ recipes.  `tokenizer`: the residual-VQ pose tokenizer (train/train_vq.py)."""


def __getattr__(name):
    if name in ("TokenizerTrainer", "train_tokenizer"):      # imports torch and, on use, the HIP library
        from . import tokenizer
        return getattr(tokenizer, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
