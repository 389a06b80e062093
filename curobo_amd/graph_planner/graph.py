"""Roadmap edges and shortest paths on the host: an undirected weighted adjacency list and Dijkstra over
``heapq`` (the reference keeps a ``networkx.Graph``, graph_planner/search/path_finder_networkx.py; networkx
is not a dependency here)."""

from __future__ import annotations

import heapq
import math
from typing import Dict, Iterable, List, Optional, Sequence, Tuple


class RoadmapGraph:
    """Undirected graph of node indices; an edge added twice keeps the later weight (networkx ``add_weighted_edges_from``)."""

    def __init__(self):
        self.adj: Dict[int, Dict[int, float]] = {}

    def reset(self) -> None:
        self.adj = {}

    def add_edges(self, edges: Iterable[Sequence]) -> None:
        """edges: (u, v, weight) triples; self loops only register the node"""
        for u, v, w in edges:
            u, v = int(u), int(v)
            self.adj.setdefault(u, {})
            self.adj.setdefault(v, {})
            if u != v:
                self.adj[u][v] = float(w)
                self.adj[v][u] = float(w)

    @property
    def num_edges(self) -> int:
        return sum(len(n) for n in self.adj.values()) // 2

    def edges(self) -> List[Tuple[int, int, float]]:
        return [(u, v, w) for u, nb in self.adj.items() for v, w in nb.items() if u < v]

    def shortest_path(self, start: int, goal: int) -> Tuple[Optional[List[int]], float]:
        """(node list from start to goal, its length), (None, inf) without a path.  Equal-length paths resolve by
        the lower node index first (heap order of (distance, node))."""
        if start not in self.adj or goal not in self.adj:
            return (None, math.inf) if start != goal else ([start], 0.0)
        dist = {start: 0.0}
        prev: Dict[int, int] = {}
        heap = [(0.0, start)]
        done = set()
        while heap:
            d, u = heapq.heappop(heap)
            if u in done:
                continue
            done.add(u)
            if u == goal:
                break
            for v, w in self.adj[u].items():
                nd = d + w
                if nd < dist.get(v, math.inf):
                    dist[v] = nd
                    prev[v] = u
                    heapq.heappush(heap, (nd, v))
        if goal not in done:
            return None, math.inf
        path = [goal]
        while path[-1] != start:
            path.append(prev[path[-1]])
        return path[::-1], dist[goal]

    def path_exists(self, start: int, goal: int) -> bool:
        return self.shortest_path(start, goal)[0] is not None
