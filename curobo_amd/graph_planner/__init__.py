"""PRM graph planner (reference ``curobo/_src/graph_planner``): ``PRMGraphPlanner``, ``PRMGraphPlannerCfg``,
``GraphPlannerResult``."""

from .graph import RoadmapGraph  # noqa: F401
from .prm import GraphFeasibility, GraphPlannerResult, PRMGraphPlanner, PRMGraphPlannerCfg  # noqa: F401
