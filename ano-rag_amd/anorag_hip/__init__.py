"""Host-side bindings of libanorag_hip.so (C ABI: include/anorag.h)."""
from ._lib import AnoragError, METRIC_IP, METRIC_L2, device_count, load  # noqa: F401
from .flat_index import FlatIndex  # noqa: F401
from .ivf_index import IVFIndex  # noqa: F401
from .graph_index import GraphIndex  # noqa: F401
from .note_graph import NoteGraph  # noqa: F401
from .topic_clustering import cluster_labels, dbscan_labels, find_optimal_eps  # noqa: F401
from .topic_clustering import analyze_clusters, cluster_cohesion, silhouette_samples, silhouette_score  # noqa: F401
from .diversity import diversify  # noqa: F401
from . import graph_quality  # noqa: F401
from .graph_quality import compute_metrics  # noqa: F401
from . import note_relations  # noqa: F401
from .note_relations import SetJoin, entity_coexistence_relations, topic_relations  # noqa: F401
from . import related_notes  # noqa: F401
from .related_notes import NoteSimilarityCalculator, related_pairs  # noqa: F401
from . import note_dedup  # noqa: F401
from .note_dedup import TfidfJoin, detect_duplicate_notes, entity_duplicates, lexical_duplicates  # noqa: F401
from .note_dedup import relabel_terms, semantic_duplicates  # noqa: F401
from . import khop_rerank  # noqa: F401
from .khop_rerank import cluster_suppression, rerank_khop  # noqa: F401
