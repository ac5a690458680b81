from .train import FusedAdamWStep, build_tables, reference_step, to_cuda, train_k_steps_cosine, train_step  # noqa: F401
