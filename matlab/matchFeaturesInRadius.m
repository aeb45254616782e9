function [indexPairs, matchMetric] = matchFeaturesInRadius(features1, features2, points2, centerPoints, radius, varargin)
%MATCHFEATURESINRADIUS libvo (MI355X) shadow: [indexPairs, matchMetric] = matchFeaturesInRadius(features1, features2, points2, centerPoints, radius, Name, Value)
%   Guided matching: row i of features1 is compared only with the rows of
%   features2 whose point (points2, N2 x 2 [x y] or an object with .Location)
%   lies within radius (a scalar, or one value per row of features1) of
%   centerPoints(i, :), the circle closed.  The ratio test and 'Unique' run
%   over those candidates alone, so this is not a filter of matchFeatures'
%   result: a repeated structure elsewhere in the image does not kill a match.
%   Guided stereo: centerPoints = the left points shifted by the expected
%   disparity; guided tracking: last frame's positions or their reprojection.
%   Options as matchFeatures: 'Unique', 'MatchThreshold' ((0, 25]), 'MaxRatio'
%   ((0, 1]); 'Method', 'Metric' and 'Prenormalized' only at their defaults;
%   anything else raises vo:matchFeaturesInRadius:options.  Everything is cast
%   to single and handed over as it lies; features must be u8-valued (SIFT
%   descriptors as extractFeatures returns them).  indexPairs is P x 2 uint32,
%   ascending in the first column; matchMetric is P x 1 single, the SSD.
    if isobject(points2) || isstruct(points2)
        points2 = points2.Location;
    end
    if isobject(centerPoints) || isstruct(centerPoints)
        centerPoints = centerPoints.Location;
    end
    if nargout > 1
        [indexPairs, matchMetric] = vo_mex('matchradius', single(features1), single(features2), single(points2), ...
                                           single(centerPoints), single(radius), varargin{:});
    else
        indexPairs = vo_mex('matchradius', single(features1), single(features2), single(points2), ...
                            single(centerPoints), single(radius), varargin{:});
    end
end
