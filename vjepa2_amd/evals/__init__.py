"""Evaluation apps on the HIP path, dispatched by name like the reference's evals/scaffold.py:13-19."""

import importlib

# eval_name -> module under this package (the reference imports evals.<eval_name>.eval)
EVALS = {"video_classification_frozen": "video_classification_frozen",
         "action_anticipation_frozen": "action_anticipation_frozen",
         "image_classification_frozen": "image_classification_frozen"}


def main(eval_name, args_eval, resume_preempt=False):
    """evals/scaffold.py:13-19: run the eval `eval_name` with its config dict."""
    name = eval_name[len("evals."):] if eval_name.startswith("evals.") else eval_name
    if name not in EVALS:
        raise NotImplementedError(f"eval {eval_name!r} is not ported to the HIP path (available: {sorted(EVALS)})")
    mod = importlib.import_module(f"{__name__}.{EVALS[name]}")
    return mod.main(args_eval=args_eval, resume_preempt=resume_preempt)
