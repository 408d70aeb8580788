from h12env.distill import StudentTeacher, StudentTeacherRecurrent
from h12env.ppo import ActorCritic, EmpiricalNormalization

__all__ = ["ActorCritic", "EmpiricalNormalization", "StudentTeacher", "StudentTeacherRecurrent"]
