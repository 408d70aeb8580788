from h12env.distill import StudentTeacher, StudentTeacherRecurrent
from h12env.ppo import ActorCritic, EmpiricalNormalization
from h12env.rnd import EmpiricalDiscountedVariationNormalization, RandomNetworkDistillation

__all__ = ["ActorCritic", "EmpiricalDiscountedVariationNormalization", "EmpiricalNormalization",
           "RandomNetworkDistillation", "StudentTeacher", "StudentTeacherRecurrent"]
