from deep_recommenders_amd.estimator.models.multi_task_learning.mixture_of_experts import MMoE  # noqa: F401
from deep_recommenders_amd.estimator.models.multi_task_learning.esmm import ESMM  # noqa: F401
