"""L0: entity model, SoA arrays and trace I/O."""
from .arrays import ClusterArrays, PodArrays, Workload, dense_rank
from .model import GPU, Cluster, Node, Pod
from .schedule import Schedule, ScheduleBatch, ScheduleError
from .time_metrics import TimeMetricsBatch
from .traces import TraceParser, TraceSuite, load_default_workload, load_suite, synthetic_workload

__all__ = ["GPU", "Node", "Cluster", "Pod", "ClusterArrays", "PodArrays", "Workload", "dense_rank",
           "Schedule", "ScheduleBatch", "ScheduleError", "TimeMetricsBatch",
           "TraceParser", "TraceSuite", "load_default_workload", "load_suite", "synthetic_workload"]
