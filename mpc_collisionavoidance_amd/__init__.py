"""MI355X-native batched SQP-RTI solver for the USV collision-avoidance OCPs of
ivanacollg/MPC_CollisionAvoidance, behind the acados_template calling convention."""
from .acados_template import (AcadosModel, AcadosOcp, AcadosOcpSolver, AcadosSim, AcadosSimSolver, BatchOcpSolver,  # noqa: F401
                              BatchSimSolver)
from . import usv_models, scenario  # noqa: F401

__all__ = ["AcadosModel", "AcadosOcp", "AcadosOcpSolver", "AcadosSim", "AcadosSimSolver", "BatchOcpSolver", "BatchSimSolver",
           "usv_models", "scenario"]
