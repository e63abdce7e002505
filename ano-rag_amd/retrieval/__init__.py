"""Drop-in for the hot-path part of the reference's ``retrieval`` package: ``hybrid_search`` (reference
retrieval/__init__.py:14-16 exports HybridSearcher from there) and ``diversity_scheduler``."""
from .diversity_scheduler import (CandidateItem, CoverageMetric, DeduplicationMethod, DiversityConfig,  # noqa: F401
                                  DiversityResult, DiversityScheduler, DiversityStrategy, create_diversity_config,
                                  create_diversity_scheduler, schedule_diverse_candidates)
from .hybrid_search import HybridSearcher, create_hybrid_searcher  # noqa: F401

__all__ = ["HybridSearcher", "create_hybrid_searcher", "DiversityScheduler", "DiversityConfig", "CandidateItem",
           "DiversityResult", "DiversityStrategy", "DeduplicationMethod", "CoverageMetric", "create_diversity_scheduler",
           "create_diversity_config", "schedule_diverse_candidates"]
