"""The reference's ``LB_D2Q9.rocket_yeast`` package: ``rocket_yeast.Rocket_Yeast`` and
``rocket_yeast_forces_only.Rocket_Yeast_Forces_Only``."""
