"""Reading a trainer checkpoint (or a train_state.pth) safely: torch.load through an unpickler that admits
tensors, plain containers, numbers, strings and argparse.Namespace, and nothing else.  Lives here so that the
trainer's command line can load a file without importing the index generator's."""
import logging

import torch

log = logging.getLogger(__name__)

# Globals a trainer checkpoint ({args, epoch, best_*, state_dict, optimizer}, trainer.py:158-166) needs beyond
# plain containers and numbers: tensor rebuild helpers, typed storages, OrderedDict, and argparse.Namespace for `args`.
_CKPT_GLOBALS = {("collections", "OrderedDict"), ("argparse", "Namespace"),
                 ("torch._utils", "_rebuild_tensor_v2"), ("torch._utils", "_rebuild_parameter"),
                 ("torch", "Size"), ("torch.storage", "UntypedStorage")} | \
                {("torch", t + "Storage") for t in ("Float", "Double", "Half", "BFloat16", "Long", "Int", "Short",
                                                    "Char", "Byte", "Bool")}


class _CheckpointPickle:
    """`pickle_module` for torch.load: the real unpickler (so protocol 4's FRAME opcode, which
    trainer.py:167 makes every checkpoint carry and torch's own weights_only unpickler rejects, is read)
    with find_class restricted to _CKPT_GLOBALS -- any other global raises instead of being imported."""
    import pickle as _pickle
    __name__ = "lcrec_amd.checkpoint_pickle"
    UnpicklingError = _pickle.UnpicklingError

    class Unpickler(_pickle.Unpickler):
        def find_class(self, module, name):
            if (module, name) in _CKPT_GLOBALS:
                return super().find_class(module, name)
            import pickle
            raise pickle.UnpicklingError(f"checkpoint names the global {module}.{name}, which is not on the "
                                         "allow-list of a trainer checkpoint (use --trust_checkpoint for your own files)")

    @classmethod
    def load(cls, fh, **kw):
        return cls.Unpickler(fh, **kw).load()

    @classmethod
    def loads(cls, data, **kw):
        import io
        return cls.Unpickler(io.BytesIO(data), **kw).load()


def load_checkpoint(ckpt_path, trust=False):
    """torch.load of a trainer checkpoint with a restricted unpickler: tensors, plain containers and
    argparse.Namespace (the `args` entry), nothing else -- a file that names any other global is refused
    with pickle.UnpicklingError, never executed.  `trust=True` (CLI: --trust_checkpoint) loads the way the
    reference does (generate_indices.py:51, full pickle): only for a file you wrote yourself."""
    if trust:
        log.warning("loading %s with the unrestricted unpickler (--trust_checkpoint)", ckpt_path)
        return torch.load(ckpt_path, map_location=torch.device("cpu"), weights_only=False)
    return torch.load(ckpt_path, map_location=torch.device("cpu"), weights_only=False, pickle_module=_CheckpointPickle)
