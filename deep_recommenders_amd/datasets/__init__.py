from .movielens import MovieLens, MovielensRanking, TFRecordFile, BytesColumn, parse_int64, parse_bytes  # noqa: F401
from .synthetic_for_multi_task import SyntheticForMultiTask  # noqa: F401
from .cora import Cora, synthetic_cora  # noqa: F401
