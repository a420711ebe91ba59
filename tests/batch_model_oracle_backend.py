"""Test-only stand-in for capi.Context.set_models_batched on the CPU oracle: the batched oracle backends with one packed MODEL per
environment. The oracle takes a packed model per call, so environment e of a batched call is the parent class's call on a fleet of
ONE (batch_task_oracle_backend.TaskRows._each) with the model of environment e in place of the context's. As in the library the plain
calls keep the context's own model, the models persist until replaced, and a batched call with another number of environments than
models is refused. Never used by the product."""
from batch_robust_oracle_backend import BatchRobustOracleContext
from batch_sample_gradient_oracle_backend import BatchSampleGradientOracleContext
from batch_task_oracle_backend import TaskBatchCeOracleContext, TaskBatchOracleContext


class ModelRows:
    """mixin in front of a backend that has TaskRows"""
    env_models = None

    def set_models_batched(self, packed_models):
        models = list(packed_models) if packed_models is not None else []
        ref = self.pm.struct
        for e, pm in enumerate(models):
            m = pm.struct
            if (m.nq, m.nv, m.nu, m.nbody, m.ngeom, m.timestep, m.integrator) != (ref.nq, ref.nv, ref.nu, ref.nbody, ref.ngeom, ref.timestep, ref.integrator):
                raise ValueError(f"set_models_batched: environment {e}: sizes or options differ from the context's model")
        self.env_models = models or None
        self.model_pushes = getattr(self, "model_pushes", []) + [None if not models else list(models)]      # for the tests

    def _each(self, call, view=False):
        models = self.env_models
        if models is None:
            return super()._each(call, view)
        if len(models) != self.E:
            raise ValueError(f"batched rollout of {self.E} environments on a context that holds {len(models)} models")
        own = self.pm

        def on_its_model(e):
            self.pm = models[e]
            try:
                return call(e)
            finally:
                self.pm = own
        return super()._each(on_its_model, view)


class ModelBatchOracleContext(ModelRows, TaskBatchOracleContext):
    pass


class ModelBatchCeOracleContext(ModelRows, TaskBatchCeOracleContext):
    pass


class ModelBatchRobustOracleContext(ModelRows, BatchRobustOracleContext):
    pass


class ModelBatchSampleGradientOracleContext(ModelRows, BatchSampleGradientOracleContext):
    pass
