from .AFs import AF_EI, AF_HF, AF_HF_Engineering, AF_LF, AF_LF_Engineering  # noqa: F401
from .BO_GP_plus import BO  # noqa: F401
from .thompson import thompson_sample  # noqa: F401
from .active_learning import select_by_variance_reduction, select_run_by_variance_reduction  # noqa: F401
from .knowledge_gradient import select_by_knowledge_gradient  # noqa: F401
